#!/usr/bin/env python3
"""Generate image_refusals.json: what every image entry point refuses, and in which order, before a device is looked for.

    python tests/golden/make_image_refusals.py

The entries are the film development, statistics, tone mapping, denoising, reprojection, temporal resolve and motion blur of
include/pyrite_gpu.h, each in its host and its _device form. Every call gets 4 x 3 buffers of zeros, 16-byte aligned, and device
number 99, which no machine has: a call that passes every check ends at "no such HIP device", with and without a GPU. A call
carries no fault, one fault, or two faults of different groups -- the pairs pin the order of an entry's checks:
  null     one pointer argument NULL (the optional ones and the tables of the development parameters included)
  param    one parameter field a step outside its range, NaN or infinite; a reserved word set; film bins 0; an unknown space
  extent   width 0, height 0, 65536 x 65536
  align    one record array moved by 4 bytes (_device forms)
  overlap  one output laid over the end of an input or of another output (the entries that check for it)
tests/test_image_refusals_cpu.py replays the file against the built library: code and pyr_last_error() text of every record."""
import ctypes as C
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from pyrite_amd import abi  # noqa: E402

OUT = os.path.join(HERE, "image_refusals.json")
W, H, BINS, SAMPLES, XYZ, DEVICE = 4, 3, 5, 6, 4, 99
PIXELS = W * H
NAN, INF = float("nan"), float("inf")
GROUPS = ("null", "param", "extent", "align", "overlap")
EXTENTS = {"width 0": (0, H), "height 0": (W, 0), "65536 x 65536": (65536, 65536)}


def below(v):
    return float(np.nextafter(np.float32(v), np.float32(-INF)))


def above(v):
    return float(np.nextafter(np.float32(v), np.float32(INF)))


def faults(target, field, *values):
    """{label: (the argument, its field, the value)}; target None: the argument is a plain word."""
    return {"%s=%r" % (field, v): (target, field, v) for v in values}


def merged(*tables):
    return {k: v for t in tables for k, v in t.items()}


def image(*names):
    return [(n, 12 * PIXELS) for n in names]


def records(*names):
    return [(n, 32 * PIXELS) for n in names]


def counts(*names):
    return [(n, 4 * PIXELS) for n in names]


P = "params"
HISTORY_FAULTS = merged(faults(P, "depth_tolerance", below(0.0), NAN, INF), faults(P, "max_history", below(1.0), NAN, INF))
RESERVED2 = merged(faults(P, "reserved[0]", 1), faults(P, "reserved[1]", 1))
DEVELOP_FAULTS = merged(faults(P, "step_size", 0.0, NAN, INF), faults(P, "xyz_scale", NAN, INF), faults(P, "sample_count", 0), faults(P, "xyz_count", 1),
                        faults(P, "xyz_min", NAN, INF), faults(P, "xyz_max", NAN, INF), faults("film", "bins", 0))
DEVELOP_TABLES = [("params.filter", 4 * SAMPLES), ("params.white_div", 4 * SAMPLES), ("params.white_mul", 4 * SAMPLES), ("params.xyz_table", 12 * XYZ)]
GRAINS = 8 * BINS * PIXELS


def develop_params():
    return abi.PyrDevelopParams(step_size=2.0, xyz_scale=1.0, sample_count=SAMPLES, xyz_count=XYZ, xyz_min=380.0, xyz_max=780.0)


# One row an operation: the arguments in the order of the declaration (the _device form takes a stream after them), the buffers
# and their bytes, the parameter block with its faults, the record arrays, whether the _device form checks for overlap.
OPS = {
    "pyr_film_develop": dict(order=["film", "grains", P, "out", "device"], inputs=[("grains", GRAINS)], outputs=[("out", 3 * PIXELS)], tables=DEVELOP_TABLES,
                             params=develop_params, faults=DEVELOP_FAULTS),
    "pyr_film_develop_linear": dict(order=["film", "grains", "grains_b", P, "space", "out", "device"], inputs=[("grains", GRAINS), ("grains_b", GRAINS)],
                                    outputs=image("out"), tables=DEVELOP_TABLES, params=develop_params, faults=merged(DEVELOP_FAULTS, faults(None, "space", 2))),
    "pyr_image_stats": dict(order=["image", "width", "height", "out", "device"], inputs=image("image"), outputs=[("out", C.sizeof(abi.PyrImageStats))]),
    "pyr_image_tonemap": dict(order=["image", "width", "height", P, "out", "device"], inputs=image("image"), outputs=[("out", 3 * PIXELS)],
                              params=lambda: abi.PyrToneParams(abi.PYR_TONE_REINHARD, 1.0, 2.0, abi.PYR_TONE_KEY, abi.PYR_TONE_PERCENTILE, abi.PYR_TONE_WHITE_PERCENTILE),
                              faults=merged(faults(P, "op", 2), faults(P, "exposure", 0.0, NAN, INF), faults(P, "white", 0.0, NAN, INF), faults(P, "key", 0.0, NAN, INF),
                                            faults(P, "percentile", 0.0, above(1.0), NAN, INF), faults(P, "white_percentile", 0.0, above(1.0), NAN, INF))),
    "pyr_image_denoise": dict(order=["a", "b", "albedo", "pixels", "width", "height", P, "out", "error_out", "device"],
                              inputs=image("a", "b", "albedo") + records("pixels"), outputs=image("out", "error_out"), records=("pixels",),
                              params=lambda: abi.PyrDenoiseParams(abi.PYR_DENOISE_RADIUS, abi.PYR_DENOISE_PATCH, abi.PYR_DENOISE_K, abi.PYR_DENOISE_EPSILON,
                                                                  abi.PYR_DENOISE_SIGMA_ALBEDO, abi.PYR_DENOISE_SIGMA_NORMAL, abi.PYR_DENOISE_SIGMA_DEPTH, 0),
                              faults=merged(faults(P, "radius", 0, 11), faults(P, "patch", 4), faults(P, "k", 0.0, NAN, INF), faults(P, "epsilon", 0.0, NAN, INF),
                                            faults(P, "sigma_albedo", NAN, INF), faults(P, "sigma_normal", NAN, INF), faults(P, "sigma_depth", NAN, INF),
                                            faults(P, "reserved", 1))),
    "pyr_image_reproject": dict(order=["current", "motion", "history", "history_motion", "history_count", "width", "height", P, "out", "count_out", "device"],
                                inputs=image("current") + records("motion") + image("history") + records("history_motion") + counts("history_count"),
                                outputs=image("out") + counts("count_out"), records=("motion", "history_motion"),
                                params=lambda: abi.PyrReprojectParams(abi.PYR_REPROJECT_DEPTH_TOLERANCE, abi.PYR_REPROJECT_MAX_HISTORY),
                                faults=merged(HISTORY_FAULTS, RESERVED2)),
    "pyr_image_temporal_resolve": dict(
        order=["current", "motion", "noise", "history", "history_motion", "history_count", "width", "height", P, "out", "count_out", "clip_out", "device"],
        inputs=image("current") + records("motion") + image("noise", "history") + records("history_motion") + counts("history_count"),
        outputs=image("out") + counts("count_out", "clip_out"), records=("motion", "history_motion"), overlap=True,
        params=lambda: abi.PyrTemporalParams(abi.PYR_REPROJECT_DEPTH_TOLERANCE, abi.PYR_REPROJECT_MAX_HISTORY, abi.PYR_TEMPORAL_RADIUS, abi.PYR_TEMPORAL_GAMMA,
                                             abi.PYR_TEMPORAL_NOISE_SCALE, abi.PYR_TEMPORAL_RESPONSE),
        faults=merged(HISTORY_FAULTS, faults(P, "radius", 0, 4), faults(P, "gamma", below(0.0), NAN, INF), faults(P, "noise_scale", below(0.0), NAN, INF),
                      faults(P, "response", below(0.0), NAN, INF), RESERVED2)),
    "pyr_image_motion_blur": dict(order=["image", "motion", "width", "height", P, "out", "device"], inputs=image("image") + records("motion"), outputs=image("out"),
                                  records=("motion",), overlap=True,
                                  params=lambda: abi.PyrMotionBlurParams(abi.PYR_MOTION_BLUR_SHUTTER, abi.PYR_MOTION_BLUR_SAMPLES, abi.PYR_MOTION_BLUR_MAX_RADIUS,
                                                                         abi.PYR_MOTION_BLUR_DEPTH_SOFTNESS, 7),
                                  faults=merged(faults(P, "shutter", 0.0, above(1.0), NAN, INF), faults(P, "samples", 0, 65), faults(P, "max_radius", 0, 65),
                                                faults(P, "depth_softness", 0.0, NAN, INF), faults(P, "reserved[0]", 1), faults(P, "reserved[1]", 1),
                                                faults(P, "reserved[2]", 1))),
}
ENTRIES = [name + form for name in OPS for form in ("", "_device")]


def fault_groups(entry):
    """{group: the faults of that group this entry can be given}, each fault a string "group: what"."""
    op, device_form = OPS[entry.replace("_device", "")], entry.endswith("_device")
    ins, outs = [n for n, _ in op["inputs"]], [n for n, _ in op["outputs"]]
    pointers = [n for n in op["order"] if n in ins + outs + ["film", P]] + [n for n, _ in op.get("tables", [])]
    found = {"null": pointers, "param": list(op.get("faults", {})), "extent": list(EXTENTS), "align": list(op.get("records", ())) if device_form else [], "overlap": []}
    if device_form and op.get("overlap"):
        found["overlap"] = ["%s over %s" % (o, i) for o in outs for i in ins] + ["%s over %s" % (a, b) for a, b in itertools.combinations(outs, 2)]
    return {group: ["%s: %s" % (group, what) for what in found[group]] for group in GROUPS}


def cases(entry):
    """No fault, every single fault, every pair of faults of two different groups."""
    groups = fault_groups(entry)
    singles = [(f,) for g in GROUPS for f in groups[g]]
    pairs = [(a, b) for g, h in itertools.combinations(GROUPS, 2) for a in groups[g] for b in groups[h]]
    return [()] + singles + pairs


def set_field(struct, field, value):
    if field.endswith("]"):
        name, index = field[:-1].split("[")
        getattr(struct, name)[int(index)] = value
    else:
        setattr(struct, field, value)


def call(lib, entry, given=()):
    """One call of `entry` with the faults `given`: (return code, pyr_last_error() text)."""
    op, device_form = OPS[entry.replace("_device", "")], entry.endswith("_device")
    sizes = dict(op["inputs"] + op["outputs"] + op.get("tables", []))
    arena = np.zeros(sum(n + 32 for n in sizes.values()) + 16, dtype=np.uint8)  # one allocation: the buffers lie in one order at any extent
    at, cursor = {}, arena.ctypes.data + (-arena.ctypes.data) % 16
    for name, n in sizes.items():
        at[name], cursor = cursor, cursor + (n + 31) // 16 * 16
    words = dict(width=W, height=H, space=abi.PYR_LINEAR_SRGB)
    blocks = {"film": abi.PyrFilmDesc(W, H, BINS, 380.0, 80.0), P: op["params"]() if "params" in op else None}
    by_group = {g: [f.split(": ", 1)[1] for f in given if f.startswith(g + ": ")] for g in GROUPS}
    for what in by_group["extent"]:
        words["width"], words["height"] = blocks["film"].width, blocks["film"].height = EXTENTS[what]
    for what in by_group["param"]:
        target, field, value = op["faults"][what]
        if target is None:
            words[field] = value
        else:
            set_field(blocks[target], field, value)
    for what in by_group["overlap"]:
        mover, under = what.split(" over ")
        at[mover] = at[under] + sizes[under] - 4  # the output starts on the last word of the other buffer
    for what in by_group["align"]:
        at[what] += 4
    for what in by_group["null"]:
        if what in blocks:
            blocks[what] = None
        else:
            at[what] = None
    if blocks[P] is not None:
        for name, _ in op.get("tables", []):
            setattr(blocks[P], name.split(".")[1], C.cast(C.c_void_p(at[name]), C.POINTER(C.c_float)))
    args = []
    for name in op["order"] + (["stream"] if device_form else []):
        if name in words:
            args.append(C.c_uint32(words[name]))
        elif name == "device":
            args.append(C.c_int(DEVICE))
        elif name == "stream":
            args.append(C.c_void_p(None))
        elif name in blocks:
            args.append(C.c_void_p(C.addressof(blocks[name]) if blocks[name] is not None else None))
        else:
            args.append(C.c_void_p(at[name]))
    code = getattr(lib, entry)(*args)
    return int(code), lib.pyr_last_error().decode("utf-8", "replace")


def load(path):
    lib = C.CDLL(path)  # called with explicit ctypes words: no argtypes, so that any pointer can be NULL or moved
    lib.pyr_last_error.restype = C.c_char_p
    return lib


def main():
    from pyrite_amd import build as gpu_build

    gpu_build.build()
    lib = load(gpu_build.OUT)
    messages, calls = [], {}
    for entry in ENTRIES:
        calls[entry] = []
        for given in cases(entry):
            code, text = call(lib, entry, given)
            if text not in messages:
                messages.append(text)
            calls[entry].append([" + ".join(given), code, messages.index(text)])
    with open(OUT, "w") as f:  # one record a line: [the faults, the return code, the index of the text in "messages"]
        f.write('{"messages": [\n' + ",\n".join(" " + json.dumps(m) for m in messages) + '\n],\n"calls": {\n')
        f.write(",\n".join(' "%s": [\n%s\n ]' % (entry, ",\n".join("  " + json.dumps(r) for r in calls[entry])) for entry in ENTRIES))
        f.write("\n}}\n")
    print("%s: %d records, %d texts" % (OUT, sum(len(v) for v in calls.values()), len(messages)))


if __name__ == "__main__":
    main()
