"""include/pyrite_gpu.h "motion records and accumulation over frames" restated in numpy float32, one rounding per operation in the
order the header writes: the pixel-centre rays of the pass, the position of a hit, the motion record of a pixel, and
pyr_image_reproject. Nothing here calls the library; the tests feed it pyr_scene_intersect's hits and
pyr_camera_world_to_cam's matrix and compare bit for bit."""
import numpy as np

f32 = np.float32
HIT_NONE = 0xFFFFFFFF
SHAPE_SPHERE, SHAPE_TRIANGLE, SHAPE_PLANE = 0, 1, 2
MOTION_HIT, MOTION_IN_FRONT, MOTION_INSIDE = 1, 2, 4
RECORD = np.dtype([("prev_x", "<f4"), ("prev_y", "<f4"), ("prev_depth", "<f4"), ("depth", "<f4"), ("shape", "<u4"), ("flags", "<u4"), ("reserved", "<u4", (2,))])
HALF, ONE, ZERO = f32(0.5), f32(1), f32(0)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def affine(m, p):
    """Rows 0..2 of the column-major 4x4 `m` applied to the points p [..., 3]: ((m0*x + m4*y) + m8*z) + m12."""
    m = np.asarray(m, dtype=f32)
    return np.stack([((m[r] * p[..., 0] + m[4 + r] * p[..., 1]) + m[8 + r] * p[..., 2]) + m[12 + r] for r in range(3)], axis=-1)


def linear(m, v):
    m = np.asarray(m, dtype=f32)
    return np.stack([(m[r] * v[..., 0] + m[4 + r] * v[..., 1]) + m[8 + r] * v[..., 2] for r in range(3)], axis=-1)


def pixel_rays(cam_to_world, view_plane, focus_distance, width, height):
    """float32 [height, width, 6]: the ray through each pixel's centre and the centre of the lens (Camera::to_view_area of the
    pixel, its middle, Camera::ray_towards with the aperture read as 0)."""
    m = np.asarray(cam_to_world, dtype=f32)
    vp, fd = f32(view_plane), f32(focus_distance)
    iw, ih = f32(width), f32(height)
    half_max = max(iw, ih) * HALF
    x, y = np.meshgrid(np.arange(width, dtype=f32), np.arange(height, dtype=f32))
    from_x, from_y = (x + -(iw * HALF)) / half_max, (y + -(ih * HALF)) / half_max
    size = ONE / half_max
    px, py = from_x + size * HALF, from_y + size * HALF
    target = np.stack([px / vp * fd, -(py / vp * fd), np.full_like(px, -fd)], axis=-1)
    unit = target * (ONE / np.sqrt(dot(target, target)))[..., None]
    origin = np.zeros(3, dtype=f32)
    o = affine(m, origin)
    w = ((m[3] * origin[0] + m[7] * origin[1]) + m[11] * origin[2]) + m[15]
    o = o * (ONE / w)
    rays = np.zeros((height, width, 6), dtype=f32)
    rays[..., :3] = o
    rays[..., 3:] = linear(m, unit)
    return rays


def hit_positions(rays, hits, spheres, planes):
    """float32 [..., 3]: the position the surface data of each hit has (zeros on a miss): o + d*t on a triangle, the point the
    sphere routine (shapes: tca, thc) and the plane routine return otherwise."""
    o, d = rays[..., :3], rays[..., 3:]
    kind, index = hits["shape"] >> 30, hits["shape"] & 0x3FFFFFFF
    hit = hits["shape"] != HIT_NONE
    P = np.where(hit[..., None], o + d * hits["distance"][..., None], ZERO).astype(f32)
    with np.errstate(all="ignore"):
        on = hit & (kind == SHAPE_SPHERE)
        if on.any():
            s = np.asarray(spheres, dtype=f32).reshape(-1, 4)[index[on]]
            c, r = s[:, :3], s[:, 3]
            l = c - o[on]
            tca = dot(l, d[on])
            d2 = dot(l, l) - tca * tca
            thc = np.sqrt(r * r - d2)
            P[on] = o[on] + d[on] * (tca - thc)[:, None]
        on = hit & (kind == SHAPE_PLANE)
        if on.any():
            pl = np.asarray(planes, dtype=f32).reshape(-1, 8)[index[on]]
            origin, normal = pl[:, :3], pl[:, 3:6]
            t = (dot(origin, normal) - dot(o[on], normal)) / dot(d[on], normal)
            P[on] = o[on] + d[on] * t[:, None]
    return P


def motion_records(rays, hits, w, view_plane, spheres=None, planes=None, previous_positions=None, previous_spheres=None):
    """RECORD [height, width] from the pass's rays [height, width, 6], their hits (structured: distance, shape, u, v), the previous
    camera's world_to_cam `w` [16] and view_plane, the scene's sphere table and planes as they are now, and the snapshot (None:
    none kept)."""
    height, width = hits.shape
    d = rays[..., 3:]
    kind, index = hits["shape"] >> 30, hits["shape"] & 0x3FFFFFFF
    hit = hits["shape"] != HIT_NONE
    with np.errstate(all="ignore"):
        Q = hit_positions(rays, hits, spheres, planes)
        on = hit & (kind == SHAPE_SPHERE)
        if previous_spheres is not None and on.any():
            now = np.asarray(spheres, dtype=f32).reshape(-1, 4)[index[on]]
            then = np.asarray(previous_spheres, dtype=f32).reshape(-1, 4)[index[on]]
            Q[on] = then[:, :3] + (Q[on] - now[:, :3]) * (then[:, 3] / now[:, 3])[:, None]
        on = hit & (kind == SHAPE_TRIANGLE)
        if previous_positions is not None and on.any():
            t = np.asarray(previous_positions, dtype=f32).reshape(-1, 3, 3)[index[on]]
            a, e1, e2 = t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
            Q[on] = (a + e1 * hits["u"][on][:, None]) + e2 * hits["v"][on][:, None]
        q = np.where(hit[..., None], affine(w, Q), linear(w, d)).astype(f32)
        zc = -q[..., 2]
        front = zc > 0
        vx, vy = (q[..., 0] / zc) * f32(view_plane), (-q[..., 1] / zc) * f32(view_plane)
        fw, fh = f32(width), f32(height)
        m = max(fw, fh) * HALF
        prev_x, prev_y = vx * m + fw * HALF, vy * m + fh * HALF
        inside = front & (prev_x >= 0) & (prev_x < fw) & (prev_y >= 0) & (prev_y < fh)
        prev_depth = np.sqrt((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2])
    rec = np.zeros((height, width), dtype=RECORD)
    rec["prev_x"], rec["prev_y"] = np.where(front, prev_x, ZERO), np.where(front, prev_y, ZERO)
    rec["prev_depth"], rec["depth"] = np.where(hit, prev_depth, ZERO), np.where(hit, hits["distance"], ZERO)
    rec["shape"] = hits["shape"]
    rec["flags"] = hit * MOTION_HIT + front * MOTION_IN_FRONT + inside * MOTION_INSIDE
    return rec


def reproject(current, motion, history=None, history_motion=None, history_count=None, depth_tolerance=0.02, max_history=32.0):
    """(out [h, w, 3], count [h, w]) of pyr_image_reproject, pixel by pixel."""
    current = np.asarray(current, dtype=f32)
    height, width, _ = current.shape
    out, count = current.copy(), np.ones((height, width), dtype=f32)
    if history is None:
        return out, count
    history, history_count = np.asarray(history, dtype=f32), np.asarray(history_count, dtype=f32)
    tol, most = f32(depth_tolerance), f32(max_history)
    fw, fh = f32(width), f32(height)
    with np.errstate(all="ignore"):
        for y in range(height):
            for x in range(width):
                r = motion[y, x]
                if not (int(r["flags"]) & MOTION_IN_FRONT) or not np.isfinite(r["prev_x"]) or not np.isfinite(r["prev_y"]):
                    continue
                gx, gy = f32(r["prev_x"] - HALF), f32(r["prev_y"] - HALF)
                x0, y0 = np.floor(gx), np.floor(gy)
                fx, fy = f32(gx - x0), f32(gy - y0)
                taps = [(x0, y0, f32((ONE - fx) * (ONE - fy))), (f32(x0 + ONE), y0, f32(fx * (ONE - fy))), (x0, f32(y0 + ONE), f32((ONE - fx) * fy)),
                        (f32(x0 + ONE), f32(y0 + ONE), f32(fx * fy))]
                Wt, Hc, N = ZERO, np.zeros(3, dtype=f32), ZERO
                for tx, ty, w in taps:
                    if not (tx >= 0 and tx < fw and ty >= 0 and ty < fh):
                        continue
                    ix, iy = int(tx), int(ty)
                    if ix >= width or iy >= height:
                        continue
                    h = history_motion[iy, ix]
                    if h["shape"] != r["shape"]:
                        continue
                    if int(r["flags"]) & MOTION_HIT:
                        if not (np.abs(f32(h["depth"] - r["prev_depth"])) <= f32(tol * np.fmax(h["depth"], r["prev_depth"]))):
                            continue
                    if not (history_count[iy, ix] > 0):
                        continue
                    if not np.isfinite(history[iy, ix]).all():
                        continue
                    Wt = f32(Wt + w)
                    Hc = (Hc + w * history[iy, ix]).astype(f32)
                    N = f32(N + f32(w * history_count[iy, ix]))
                if not (Wt > 0):
                    continue
                H = (Hc / Wt).astype(f32)
                n = f32(np.fmin(f32(N / Wt), most))
                out[y, x] = (H + (current[y, x] - H) / f32(n + ONE)).astype(f32)
                count[y, x] = f32(n + ONE)
    return out, count
