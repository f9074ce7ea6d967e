"""First-hit feature images (include/pyrite_gpu.h "first-hit feature images"): what Renderer.features and
Session.features return, the 8-bit encodings of the normal and depth images, and the --features flags of the command line. The
encodings are pure functions of the arrays; pyrite_host.cpp's encode_normal_image / encode_depth_image write the same bytes."""
import numpy as np

from .film import Film

f32 = np.float32
RECORD = np.dtype([("normal", "<f4", (3,)), ("depth", "<f4"), ("coverage", "<f4"), ("shape", "<u4"), ("material", "<u4"), ("reserved", "<u4")])
assert RECORD.itemsize == 32


class Features:
    """`.albedo` is a Film of `albedo_bins` bins (develop and the PNG writer apply); `.normal` [h, w, 3], `.depth`, `.coverage`
    [h, w] float32 and `.shape`, `.material` [h, w] uint32 are views of `.records`, the PyrFeaturePixel array [h, w]."""

    def __init__(self, width, height, albedo_bins=16, wavelength_span=(380.0, 780.0)):
        self.albedo = Film(width, height, albedo_bins, wavelength_span)
        self.records = np.zeros((int(height), int(width)), dtype=RECORD)

    normal = property(lambda self: self.records["normal"])
    depth = property(lambda self: self.records["depth"])
    coverage = property(lambda self: self.records["coverage"])
    shape = property(lambda self: self.records["shape"])
    material = property(lambda self: self.records["material"])


def _to_byte(v):
    """f32 in [0, 1] -> uint8 by (uint8)(v * 255 + 0.5); NaN and anything below 0 give 0, anything above 1 gives 255."""
    v = np.asarray(v, dtype=f32)
    v = np.where(v > 0, v, f32(0))
    v = np.where(v < 1, v, f32(1))
    return (v * f32(255) + f32(0.5)).astype(f32).astype(np.uint8)


def encode_normal(normal, coverage):
    """uint8 [h, w, 3]: round(255 * (0.5 * n + 0.5)) per channel in f32; pixels with coverage 0 are black."""
    normal, coverage = np.asarray(normal, dtype=f32), np.asarray(coverage, dtype=f32)
    rgb = _to_byte(f32(0.5) * normal + f32(0.5))
    rgb[~(coverage > 0)] = 0
    return rgb


def encode_depth(depth, coverage):
    """uint8 [h, w, 3], grey: linear between the smallest and the largest depth over the pixels with coverage > 0, near is white;
    coverage 0 is black. An image of one depth is white where it is covered."""
    depth, coverage = np.asarray(depth, dtype=f32), np.asarray(coverage, dtype=f32)
    covered = coverage > 0
    out = np.zeros(depth.shape + (3,), dtype=np.uint8)
    if not covered.any():
        return out
    lo, hi = f32(depth[covered].min()), f32(depth[covered].max())
    with np.errstate(all="ignore"):
        v = (hi - depth) / f32(hi - lo) if hi > lo else np.ones_like(depth)
    grey = _to_byte(v)
    grey[~covered] = 0
    out[...] = grey[..., None]
    return out


def features_flag_problem(features, features_grid):
    """What is wrong with --features / --features-grid, in the words pyrite_host_tool uses too, or None."""
    if features_grid is not None and not features:
        return "--features-grid needs --features"
    if features_grid is not None and not 1 <= features_grid <= 8:
        return "--features-grid must be 1 to 8"
    return None


def write_feature_images(prefix, features, filter=None, white=None, device=0):
    """PREFIX_albedo.png (the albedo film developed with the project's settings, step 2), PREFIX_normal.png, PREFIX_depth.png."""
    from .develop import develop, save_png

    save_png(prefix + "_albedo.png", develop(features.albedo, filter=filter, white=white, device=device))
    save_png(prefix + "_normal.png", encode_normal(features.normal, features.coverage))
    save_png(prefix + "_depth.png", encode_depth(features.depth, features.coverage))
