"""P(rest, ranges, poses): what pyr_scene_pose computes, restated in vectorised numpy -- independent of
pyrite_amd/csrc/pose_rules.h. Every operation is one IEEE f32 operation on float32 arrays, in the order of compiler.py's
_transform_point, _transform_vector, _quat_rotate, _normalize and _quat_from_cols; numpy never fuses a multiply with an add.

    rest    dict of float32 arrays: positions [n,9], normals [n,9], frames [n,12] or None, spheres [m,4]
    ranges  list of dicts with first_triangle, num_triangles, first_sphere, num_spheres
    poses   {object index: (matrix | None, scale)}; a matrix is 4x4 as on paper or 16 floats column-major; absent = identity
"""
import numpy as np

f32 = np.float32
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1], dtype=f32)


def column_major(matrix):
    if matrix is None:
        return IDENTITY.copy()
    m = np.asarray(matrix, dtype=f32)
    if m.shape == (4, 4):
        m = m.T
    return np.ascontiguousarray(m, dtype=f32).reshape(16)


def is_identity(m, scale):
    return bool(np.all(m == IDENTITY)) and f32(scale) == f32(1.0)


def transform_vector(m, v):
    x = m[0] * v[:, 0] + m[4] * v[:, 1] + m[8] * v[:, 2]
    y = m[1] * v[:, 0] + m[5] * v[:, 1] + m[9] * v[:, 2]
    z = m[2] * v[:, 0] + m[6] * v[:, 1] + m[10] * v[:, 2]
    return np.stack([x, y, z], axis=1).astype(f32)


def transform_point(m, p):  # w is exactly 1 for a last row 0,0,0,1: the division changes no bit
    x = m[0] * p[:, 0] + m[4] * p[:, 1] + m[8] * p[:, 2] + m[12]
    y = m[1] * p[:, 0] + m[5] * p[:, 1] + m[9] * p[:, 2] + m[13]
    z = m[2] * p[:, 0] + m[6] * p[:, 1] + m[10] * p[:, 2] + m[14]
    return np.stack([x, y, z], axis=1).astype(f32)


def normalize(v):
    mag = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2], dtype=f32)
    k = f32(1.0) / mag
    return (v * k[:, None]).astype(f32)


def cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1).astype(f32)


def quat_rotate(q, vec):
    v = q[:, 1:4]
    tmp = cross(v, vec) + vec * q[:, 0:1]
    return (cross(v, tmp) * f32(2.0) + vec).astype(f32)


def quat_from_cols(c0, c1, c2):
    m00, m01, m02 = c0[:, 0], c0[:, 1], c0[:, 2]
    m10, m11, m12 = c1[:, 0], c1[:, 1], c1[:, 2]
    m20, m21, m22 = c2[:, 0], c2[:, 1], c2[:, 2]
    half, one = f32(0.5), f32(1.0)
    trace = m00 + m11 + m22
    out = np.zeros((len(c0), 4), dtype=f32)
    first = trace >= 0
    second = ~first & (m00 > m11) & (m00 > m22)
    third = ~first & ~second & (m11 > m22)
    fourth = ~first & ~second & ~third
    with np.errstate(all="ignore"):
        s = np.sqrt(one + trace, dtype=f32)
        w, s = half * s, half / s
        a = np.stack([w, (m12 - m21) * s, (m20 - m02) * s, (m01 - m10) * s], axis=1)
        s = np.sqrt((m00 - m11 - m22) + one, dtype=f32)
        x, s = half * s, half / s
        b = np.stack([(m12 - m21) * s, x, (m10 + m01) * s, (m02 + m20) * s], axis=1)
        s = np.sqrt((m11 - m00 - m22) + one, dtype=f32)
        y, s = half * s, half / s
        c = np.stack([(m20 - m02) * s, (m10 + m01) * s, y, (m21 + m12) * s], axis=1)
        s = np.sqrt((m22 - m00 - m11) + one, dtype=f32)
        z, s = half * s, half / s
        d = np.stack([(m01 - m10) * s, (m02 + m20) * s, (m21 + m12) * s, z], axis=1)
    for mask, value in ((first, a), (second, b), (third, c), (fourth, d)):
        out[mask] = value[mask]
    return out


def pose_arrays(rest, ranges, poses):
    """The posed arrays, in rest's layout. Primitives in no range, and objects posed by exactly the identity with scale 1, are
    copies of rest."""
    out = {k: (None if v is None else np.array(v, dtype=f32, copy=True)) for k, v in rest.items()}
    has_frames = rest.get("frames") is not None and len(rest["frames"])
    for index, r in enumerate(ranges):
        matrix, scale = poses.get(index, (None, 1.0))
        m, scale = column_major(matrix), f32(scale)
        if is_identity(m, scale):
            continue
        t0, tn = r.get("first_triangle", 0), r.get("num_triangles", 0)
        if tn:
            p = rest["positions"][t0:t0 + tn].reshape(-1, 3).astype(f32)
            n = rest["normals"][t0:t0 + tn].reshape(-1, 3).astype(f32)
            p = (p * scale).astype(f32)
            posed_n = normalize(transform_vector(m, n))
            if has_frames:
                q = rest["frames"][t0:t0 + tn].reshape(-1, 4).astype(f32)
                ex = np.broadcast_to(np.array([1, 0, 0], dtype=f32), n.shape)
                ey = np.broadcast_to(np.array([0, 1, 0], dtype=f32), n.shape)
                x = normalize(transform_vector(m, quat_rotate(q, ex)))
                y = normalize(transform_vector(m, quat_rotate(q, ey)))
                out["frames"][t0:t0 + tn] = quat_from_cols(x, y, posed_n).reshape(-1, 12)
            out["normals"][t0:t0 + tn] = posed_n.reshape(-1, 9)
            out["positions"][t0:t0 + tn] = transform_point(m, p).reshape(-1, 9)
        s0, sn = r.get("first_sphere", 0), r.get("num_spheres", 0)
        if sn:
            s = rest["spheres"][s0:s0 + sn].astype(f32)
            radius = (s[:, 3] * scale).astype(f32)
            centre = transform_point(m, (s[:, :3] * scale).astype(f32))
            out["spheres"][s0:s0 + sn] = np.concatenate([centre, radius[:, None]], axis=1)
    return out


def lamp_areas(arrays, lamps):
    """pack_lamp's surface areas (scene_pack.cpp) for shape lamps, unfused f32: 0.5 * sqrt(|a x b|^2) and r*r*4*pi. `lamps`: a list of
    (shape_kind, shape_index) with shape_kind 0 = sphere, 1 = triangle (PYR_SHAPE_*)."""
    areas = []
    for kind, index in lamps:
        if kind == 0:
            r = f32(arrays["spheres"][index, 3])
            areas.append(f32(f32(f32(r * r) * f32(4.0)) * f32(3.14159265358979323846)))
        else:
            p = arrays["positions"][index].astype(f32)
            a, b = (p[3:6] - p[0:3]).astype(f32), (p[6:9] - p[0:3]).astype(f32)
            c = cross(a[None], b[None])[0]
            areas.append(f32(f32(0.5) * np.sqrt(f32(f32(c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]), dtype=f32)))
    return np.array(areas, dtype=f32)
