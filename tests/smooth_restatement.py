"""N(P_object(S(M(rest)))): what a smoothing adds to pyr_scene_pose, pyr_scene_skin and pyr_scene_morph,
restated in vectorised numpy from the contract in include/pyrite_gpu.h -- independent of pyrite_amd/csrc/pose_rules.h. Every
operation is one IEEE f32 operation on float32 arrays, cast back to float32 after each; the primitives are those of
tests/pose_restatement.py. It is applied to what morph_restatement / skin_restatement / pose_restatement leave.

    arrays     the arrays after the morph, the skin and the pose, in rest's layout
    rest       the rest pose (the orientation of every triangle is decided there)
    ranges     as pose_restatement.pose_arrays takes them
    smoothing  {object index: integer labels [n,3]}: corners of the object with equal labels share a normal
"""
import numpy as np

from morph_restatement import dot, outside
from pose_restatement import cross, f32, normalize, quat_from_cols, quat_rotate
from skin_restatement import skin_arrays
import morph_restatement


def weld(positions, normals):
    """Labels [n,3]: two corners share one exactly when the bits of position and normal agree in all six words."""
    words = np.concatenate([np.ascontiguousarray(positions, dtype=f32).reshape(-1, 3), np.ascontiguousarray(normals, dtype=f32).reshape(-1, 3)], axis=1).view(np.uint32)
    _, inverse = np.unique(words, axis=0, return_inverse=True)
    return inverse.reshape(-1, 3).astype(np.uint32)


def groups_of(ids):
    """(group [C], order [C], begin [G+1]) of an object's labels: `group` numbers the groups by their first corner, ascending;
    `order` lists the corners group by group, ascending within a group; `begin` is where each group's corners begin in `order`."""
    flat = np.asarray(ids).reshape(-1)
    _, first, inverse = np.unique(flat, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    group = rank[inverse.reshape(-1)]
    order = np.argsort(group, kind="stable")
    begin = np.concatenate([[0], np.cumsum(np.bincount(group, minlength=len(first)))])
    return group, order, begin


def face_vectors(positions):
    """cross(p1 - p0, p2 - p0) per triangle, [n,3]."""
    p = positions.reshape(-1, 3, 3).astype(f32)
    return cross((p[:, 1] - p[:, 0]).astype(f32), (p[:, 2] - p[:, 0]).astype(f32))


def negated(rest_positions, rest_normals):
    """The triangles wound against their rest normals: d < 0 with r = (n0 + n1) + n2 and d = (c.x*r.x + c.y*r.y) + c.z*r.z."""
    c = face_vectors(rest_positions)
    n = rest_normals.reshape(-1, 3, 3).astype(f32)
    r = ((n[:, 0] + n[:, 1]).astype(f32) + n[:, 2]).astype(f32)
    with np.errstate(all="ignore"):
        return dot(c, r) < f32(0.0)


def group_sums(c, order, begin):
    """m per group: the first corner's triangle's c, then m = m + c for each further corner in ascending corner order. One
    vectorised addition per rank within the groups, so every group's additions happen in its own order."""
    sizes = np.diff(begin)
    m = c[order[begin[:-1]] // 3].astype(f32)
    for r in range(1, int(sizes.max()) if len(sizes) else 0):
        has = sizes > r
        m[has] = (m[has] + c[order[begin[:-1][has] + r] // 3]).astype(f32)
    return m


def rebuilt_frames(q, n):
    """The Gram-Schmidt of pyr_scene_set_morphs: x first, then y, q' = quat_from_cols(x, y, n'). Returns (q', the lanes outside)."""
    rx = quat_rotate(q, np.broadcast_to(np.array([1, 0, 0], dtype=f32), n.shape))
    ry = quat_rotate(q, np.broadcast_to(np.array([0, 1, 0], dtype=f32), n.shape))
    d = dot(rx, n)
    x = (rx - (n * d[:, None]).astype(f32)).astype(f32)
    bad = outside(dot(x, x))
    x = normalize(x)
    e, f = dot(ry, n), dot(ry, x)
    y = ((ry - (n * e[:, None]).astype(f32)).astype(f32) - (x * f[:, None]).astype(f32)).astype(f32)
    bad = bad | outside(dot(y, y))
    y = normalize(y)
    return quat_from_cols(x, y, n), bad


def smoothed(arrays, rest, ranges, smoothing):
    """(N(arrays), flag, squared lengths): `arrays` with the normals and frames of every smoothed object recomputed from its
    positions; 4 if any squared length that is normalised lies outside [1e-30, 1e30], else 0; and every such squared length."""
    out = {k: (None if v is None else np.array(v, dtype=f32, copy=True)) for k, v in arrays.items()}
    has_frames = arrays.get("frames") is not None and len(arrays["frames"])
    flag, lengths = 0, []
    for index in sorted(smoothing):
        t0, tn = ranges[index]["first_triangle"], ranges[index]["num_triangles"]
        ids = np.asarray(smoothing[index])
        assert ids.shape == (tn, 3)
        group, order, begin = groups_of(ids)
        with np.errstate(all="ignore"):
            c = face_vectors(arrays["positions"][t0:t0 + tn])
            flip = negated(rest["positions"][t0:t0 + tn], rest["normals"][t0:t0 + tn])
            c[flip] = -c[flip]
            m = group_sums(c, order, begin)[group]  # per corner
            s = dot(m, m)
            bad = outside(s)
            lengths.append(s)
            n = normalize(m)
            if has_frames:
                q, worse = rebuilt_frames(arrays["frames"][t0:t0 + tn].reshape(-1, 4).astype(f32), n)
                out["frames"][t0:t0 + tn] = q.reshape(-1, 12)
                bad = bad | worse
        out["normals"][t0:t0 + tn] = n.reshape(-1, 9)
        if bool(bad.any()):
            flag |= 4
    return out, flag, (np.concatenate(lengths) if lengths else np.zeros(0, dtype=f32))


def smooth_arrays(rest, ranges, smoothing, morphs=None, weights=None, skins=None, joints=None, poses=None):
    """The arrays a frame leaves, in rest's layout: the morphs, then the skins, then every object's pose, then the smoothing."""
    arrays, _ = morph_restatement.morphed(rest, ranges, morphs or {}, weights or {})
    arrays = skin_arrays(arrays, ranges, skins or {}, joints or {}, poses or {})
    return smoothed(arrays, rest, ranges, smoothing)[0]


def smooth_flag(rest, ranges, smoothing, morphs=None, weights=None, skins=None, joints=None, poses=None):
    arrays, first = morph_restatement.morphed(rest, ranges, morphs or {}, weights or {})
    arrays = skin_arrays(arrays, ranges, skins or {}, joints or {}, poses or {})
    return first | smoothed(arrays, rest, ranges, smoothing)[1]
