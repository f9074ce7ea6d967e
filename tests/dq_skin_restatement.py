"""P_object(S(rest, bindings, J)) where a skin may blend its joints as dual quaternions (pyr_scene_set_skin_blend, DESIGN.md section
9s), restated in vectorised numpy from the rule in include/pyrite_gpu.h -- independent of pyrite_amd/csrc/pose_rules.h. Every
operation is one IEEE f32 operation on float32 arrays, in the order the header writes it; the primitives are those of
tests/pose_restatement.py and the linear blend is tests/skin_restatement.py's.

    rest, ranges, poses, joints   as skin_restatement.skin_arrays takes them
    skins    as there, each dict with an optional blend="linear" | "dual_quaternion" (absent: linear)
"""
import numpy as np

from pose_restatement import IDENTITY, f32, normalize, pose_arrays, quat_from_cols, quat_rotate, transform_point, transform_vector
from skin_restatement import blend as blend_linear, joint_table

HALF, ONE, TWO = f32(0.5), f32(1.0), f32(2.0)


def dot4(a, b):
    return (((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]).astype(f32) + a[:, 2] * b[:, 2]).astype(f32) + a[:, 3] * b[:, 3]).astype(f32)


def joint_dual_quaternions(table):
    """[J,8] = (r, d) of a [J,16] column-major joint table: r the renormalised quaternion of the upper 3x3, d = 0.5 * (0,t) * r."""
    table = np.asarray(table, dtype=f32)
    r = quat_from_cols(table[:, 0:3], table[:, 4:7], table[:, 8:11])
    with np.errstate(all="ignore"):
        k = (ONE / np.sqrt(dot4(r, r), dtype=f32)).astype(f32)
    r = (r * k[:, None]).astype(f32)
    r0, r1, r2, r3 = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    t0, t1, t2 = table[:, 12], table[:, 13], table[:, 14]
    d0 = f32(-0.5) * ((t0 * r1 + t1 * r2) + t2 * r3)
    d1 = HALF * ((t0 * r0 + t1 * r3) - t2 * r2)
    d2 = HALF * ((t1 * r0 + t2 * r1) - t0 * r3)
    d3 = HALF * ((t0 * r2 + t2 * r0) - t1 * r1)
    return np.stack([r0, r1, r2, r3, d0, d1, d2, d3], axis=1).astype(f32)


def signed_weights(quats, indices, weights):
    """[V,4]: w0 and, for k = 1..3, wk negated where dot4(r[j0], r[jk]) < 0."""
    j, w = np.asarray(indices).reshape(-1, 4).astype(np.int64), np.asarray(weights, dtype=f32).reshape(-1, 4)
    pivot = quats[j[:, 0], :4]
    out = w.copy()
    for k in (1, 2, 3):
        out[:, k] = np.where(dot4(pivot, quats[j[:, k], :4]) < 0, -w[:, k], w[:, k])
    return out


def blend_dual_quaternions(quats, indices, weights):
    """(one matrix per vertex [16, V], the vertices that raise bit 3) from a [J,8] table of unit dual quaternions."""
    quats = np.asarray(quats, dtype=f32)
    j = np.asarray(indices).reshape(-1, 4).astype(np.int64)
    w = signed_weights(quats, indices, weights)
    q = [quats[j[:, k]] for k in range(4)]
    e = ((w[:, 0:1] * q[0] + w[:, 1:2] * q[1]).astype(f32) + w[:, 2:3] * q[2]).astype(f32) + w[:, 3:4] * q[3]
    e = e.astype(f32)
    s = dot4(e[:, :4], e[:, :4])
    bad = ~((s >= f32(1e-30)) & (s <= f32(1e30)))
    with np.errstate(all="ignore"):
        k = (ONE / np.sqrt(s, dtype=f32)).astype(f32)
        e = (e * k[:, None]).astype(f32)
        r0, x, y, z, d0, d1, d2, d3 = (e[:, i] for i in range(8))
        x2, y2, z2 = x + x, y + y, z + z
        xx2, xy2, xz2, yy2, yz2, zz2 = x2 * x, x2 * y, x2 * z, y2 * y, y2 * z, z2 * z
        sx2, sy2, sz2 = x2 * r0, y2 * r0, z2 * r0
        b = np.zeros((16, len(j)), dtype=f32)
        b[0], b[1], b[2] = ONE - yy2 - zz2, xy2 + sz2, xz2 - sy2
        b[4], b[5], b[6] = xy2 - sz2, ONE - xx2 - zz2, yz2 + sx2
        b[8], b[9], b[10] = xz2 + sy2, yz2 - sx2, ONE - xx2 - yy2
        b[12] = TWO * (((d1 * r0 - d0 * x) - d2 * z) + d3 * y)
        b[13] = TWO * (((d2 * r0 - d0 * y) + d1 * z) - d3 * x)
        b[14] = TWO * (((d3 * r0 - d0 * z) - d1 * y) + d2 * x)
    b[15] = ONE
    return b, bad


def blend_of(skin):
    return skin.get("blend", "linear")


def vertex_matrices(skin, table):
    """(B [16, V], the vertices that raise bit 3) of one skin under its [J,16] joint table."""
    if blend_of(skin) == "dual_quaternion":
        return blend_dual_quaternions(joint_dual_quaternions(table), skin["joints"], skin["weights"])
    return blend_linear(table, skin["joints"], skin["weights"]), np.zeros(np.asarray(skin["joints"]).size // 4, dtype=bool)


def dq_skinned(rest, ranges, skins, joints):
    """(S(rest, bindings, J), whether any vertex raises bit 3): rest with every skinned object's triangles moved under its skin's
    blend; a skin whose joints are all exactly the identity is a copy of rest."""
    out = {k: (None if v is None else np.array(v, dtype=f32, copy=True)) for k, v in rest.items()}
    has_frames = rest.get("frames") is not None and len(rest["frames"])
    raised = False
    for index in sorted(skins):
        skin = skins[index]
        table = joint_table(joints.get(index), skin["num_joints"])
        if bool(np.all(table == IDENTITY)):
            continue
        t0, tn = ranges[index]["first_triangle"], ranges[index]["num_triangles"]
        b, bad = vertex_matrices(skin, table)
        raised = raised or bool(bad.any())
        p = rest["positions"][t0:t0 + tn].reshape(-1, 3).astype(f32)
        n = rest["normals"][t0:t0 + tn].reshape(-1, 3).astype(f32)
        p = (p * ONE).astype(f32)  # Shape::scale by 1.0f
        with np.errstate(all="ignore"):
            moved_n = normalize(transform_vector(b, n))
            if has_frames:
                q = rest["frames"][t0:t0 + tn].reshape(-1, 4).astype(f32)
                ex = np.broadcast_to(np.array([1, 0, 0], dtype=f32), n.shape)
                ey = np.broadcast_to(np.array([0, 1, 0], dtype=f32), n.shape)
                x = normalize(transform_vector(b, quat_rotate(q, ex)))
                y = normalize(transform_vector(b, quat_rotate(q, ey)))
                out["frames"][t0:t0 + tn] = quat_from_cols(x, y, moved_n).reshape(-1, 12)
            out["normals"][t0:t0 + tn] = moved_n.reshape(-1, 9)
            out["positions"][t0:t0 + tn] = transform_point(b, p).reshape(-1, 9)
    return out, raised


def dq_skin_arrays(rest, ranges, skins, joints, poses=None):
    """The arrays pyr_scene_skin leaves, in rest's layout: the skins first, each under its own blend, then every object's pose."""
    return pose_arrays(dq_skinned(rest, ranges, skins, joints)[0], ranges, poses or {})


def is_rotation(m):
    """pyr_scene_skin's test of one column-major joint matrix of a dual-quaternion skin, in f32 and its three-term order."""
    m = np.asarray(m, dtype=f32).reshape(16)
    c = [m[0:3], m[4:7], m[8:11]]
    dot = lambda a, b: f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))  # noqa: E731
    for i in range(3):
        if not abs(f32(dot(c[i], c[i]) - ONE)) <= f32(1e-3):
            return False
    for i, k in ((0, 1), (0, 2), (1, 2)):
        if not abs(dot(c[i], c[k])) <= f32(1e-3):
            return False
    a, b = c[0], c[1]
    x = [f32(f32(a[1] * b[2]) - f32(a[2] * b[1])), f32(f32(a[2] * b[0]) - f32(a[0] * b[2])), f32(f32(a[0] * b[1]) - f32(a[1] * b[0]))]
    return bool(dot(x, c[2]) > 0)
