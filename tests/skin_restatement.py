"""P_object(S(rest, bindings, J)): what pyr_scene_skin computes, restated in vectorised numpy -- independent of
pyrite_amd/csrc/pose_rules.h. Every operation is one IEEE f32 operation on float32 arrays; the primitives are those of
tests/pose_restatement.py, called with one matrix per vertex (m[k] is then a vector over the vertices), and pose_arrays applies the
object's pose to the skinned arrays afterwards.

    rest, ranges, poses   as pose_restatement.pose_arrays takes them
    skins    {object index: dict(joints uint16 [T,3,4], weights float32 [T,3,4], num_joints J)}
    joints   {object index: [J,4,4] as on paper or [J,16] column-major}; absent = every joint the identity
"""
import numpy as np

from pose_restatement import IDENTITY, f32, normalize, pose_arrays, quat_from_cols, quat_rotate, transform_point, transform_vector

UPPER_ROWS = (0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14)


def joint_table(table, num_joints):
    """[J,16] column-major float32."""
    if table is None:
        return np.tile(IDENTITY, (num_joints, 1))
    t = np.asarray(table, dtype=f32)
    if t.ndim == 3:
        t = t.transpose(0, 2, 1)
    t = np.ascontiguousarray(t, dtype=f32).reshape(len(t), 16)
    assert len(t) == num_joints
    return t


def blend(table, indices, weights):
    """One matrix per vertex, [16, V]: entry e is ((w0*J[j0][e] + w1*J[j1][e]) + w2*J[j2][e]) + w3*J[j3][e]; last row 0,0,0,1."""
    j, w = np.asarray(indices).reshape(-1, 4).astype(np.int64), np.asarray(weights, dtype=f32).reshape(-1, 4)
    b = np.zeros((16, len(j)), dtype=f32)
    b[15] = f32(1.0)
    for e in UPPER_ROWS:
        column = table[:, e]
        first = (w[:, 0] * column[j[:, 0]]).astype(f32)
        second = (w[:, 1] * column[j[:, 1]]).astype(f32)
        third = (w[:, 2] * column[j[:, 2]]).astype(f32)
        fourth = (w[:, 3] * column[j[:, 3]]).astype(f32)
        b[e] = (((first + second).astype(f32) + third).astype(f32) + fourth).astype(f32)
    return b


def skinned(rest, ranges, skins, joints):
    """S(rest, bindings, J): rest with every skinned object's triangles moved; a skin whose joints are all exactly the identity is a
    copy of rest."""
    out = {k: (None if v is None else np.array(v, dtype=f32, copy=True)) for k, v in rest.items()}
    has_frames = rest.get("frames") is not None and len(rest["frames"])
    for index in sorted(skins):
        skin = skins[index]
        table = joint_table(joints.get(index), skin["num_joints"])
        if bool(np.all(table == IDENTITY)):
            continue
        t0, tn = ranges[index]["first_triangle"], ranges[index]["num_triangles"]
        b = blend(table, skin["joints"], skin["weights"])
        p = rest["positions"][t0:t0 + tn].reshape(-1, 3).astype(f32)
        n = rest["normals"][t0:t0 + tn].reshape(-1, 3).astype(f32)
        p = (p * f32(1.0)).astype(f32)  # Shape::scale by 1.0f
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
    return out


def skin_arrays(rest, ranges, skins, joints, poses=None):
    """The arrays pyr_scene_skin leaves, in rest's layout: the skins first, then every object's pose on the skinned arrays."""
    return pose_arrays(skinned(rest, ranges, skins, joints), ranges, poses or {})
