"""P_object(S(M(rest, targets, w), bindings, J)): what pyr_scene_morph computes, restated in vectorised numpy
from the contract in include/pyrite_gpu.h -- independent of pyrite_amd/csrc/pose_rules.h. Every operation is one IEEE f32 operation
on float32 arrays, cast back to float32 after each; the primitives are those of tests/pose_restatement.py, and skin_arrays applies
the skins and the objects' poses to the morphed arrays afterwards.

    rest, ranges, poses   as pose_restatement.pose_arrays takes them
    morphs   {object index: dict(positions float32 [T,n,3,3], normals float32 [T,n,3,3] | None)}
    weights  {object index: [T]}; absent = every weight zero
    skins, joints         as skin_restatement.skin_arrays takes them
"""
import numpy as np

from pose_restatement import f32, normalize, quat_from_cols, quat_rotate
from skin_restatement import skin_arrays

LOW, HIGH = f32(1.0e-30), f32(1.0e30)


def weights_of(weights, index, num_targets):
    w = np.zeros(num_targets, dtype=f32) if weights.get(index) is None else np.asarray(weights[index], dtype=f32).reshape(-1)
    assert len(w) == num_targets
    return w


def dot(a, b):
    first = (a[:, 0] * b[:, 0]).astype(f32)
    second = (a[:, 1] * b[:, 1]).astype(f32)
    third = (a[:, 2] * b[:, 2]).astype(f32)
    return ((first + second).astype(f32) + third).astype(f32)


def outside(s):
    """The lanes that raise bit 1 of the flag word: !(s >= 1e-30f && s <= 1e30f)."""
    return ~((s >= LOW) & (s <= HIGH))


def accumulated(start, deltas, w):
    """start + w[t] * deltas[t] over the active targets in ascending t, [V,3]; an inactive target is not touched."""
    out = start.astype(f32)
    for t in range(len(w)):
        if w[t] == f32(0.0):
            continue
        out = (out + (w[t] * deltas[t].reshape(-1, 3).astype(f32)).astype(f32)).astype(f32)
    return out


def morphed(rest, ranges, morphs, weights):
    """(M(rest, targets, w), flag): rest with every morphed object's triangles moved, and 2 if any squared length that is normalised
    lies outside [1e-30, 1e30], else 0. A morph with no active target is a copy of rest."""
    out = {k: (None if v is None else np.array(v, dtype=f32, copy=True)) for k, v in rest.items()}
    has_frames = rest.get("frames") is not None and len(rest["frames"])
    flag = 0
    for index in sorted(morphs):
        morph = morphs[index]
        w = weights_of(weights, index, len(morph["positions"]))
        if not np.any(w != f32(0.0)):
            continue
        t0, tn = ranges[index]["first_triangle"], ranges[index]["num_triangles"]
        p = rest["positions"][t0:t0 + tn].reshape(-1, 3).astype(f32)
        out["positions"][t0:t0 + tn] = accumulated(p, morph["positions"], w).reshape(-1, 9)
        if morph.get("normals") is None:
            continue
        with np.errstate(all="ignore"):
            m = accumulated(rest["normals"][t0:t0 + tn].reshape(-1, 3).astype(f32), morph["normals"], w)
            bad = outside(dot(m, m))
            n = normalize(m)
            if has_frames:
                q = rest["frames"][t0:t0 + tn].reshape(-1, 4).astype(f32)
                rx = quat_rotate(q, np.broadcast_to(np.array([1, 0, 0], dtype=f32), n.shape))
                ry = quat_rotate(q, np.broadcast_to(np.array([0, 1, 0], dtype=f32), n.shape))
                d = dot(rx, n)
                x = (rx - (n * d[:, None]).astype(f32)).astype(f32)
                bad = bad | outside(dot(x, x))
                x = normalize(x)
                e, f = dot(ry, n), dot(ry, x)
                y = ((ry - (n * e[:, None]).astype(f32)).astype(f32) - (x * f[:, None]).astype(f32)).astype(f32)
                bad = bad | outside(dot(y, y))
                y = normalize(y)
                out["frames"][t0:t0 + tn] = quat_from_cols(x, y, n).reshape(-1, 12)
        out["normals"][t0:t0 + tn] = n.reshape(-1, 9)
        if bool(bad.any()):
            flag |= 2
    return out, flag


def morph_arrays(rest, ranges, morphs, weights, skins=None, joints=None, poses=None):
    """The arrays pyr_scene_morph leaves, in rest's layout: the morphs first, then the skins, then every object's pose."""
    arrays, _ = morphed(rest, ranges, morphs, weights)
    return skin_arrays(arrays, ranges, skins or {}, joints or {}, poses)


def morph_flag(rest, ranges, morphs, weights):
    return morphed(rest, ranges, morphs, weights)[1]
