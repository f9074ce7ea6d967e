"""The firefly clamp without a GPU (include/pyrite_gpu.h "despeckle"): the new names of the ABI in the header,
abi.py and the library, every argument check before a device is looked for, the C++ wrappers through a stand-alone program, the
flags of the two command lines, the kernel's tile addressing under the sanitizers in a program of its own, the kernel's resources
from the compiler's metadata, and the numpy restatement (tests/despeckle_restatement.py, which tests/test_gpu_despeckle.py holds the
kernel against) on properties of the rule itself."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import despeckle_restatement as R
from pyrite_amd import abi, develop
from pyrite_amd import build as gpu_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pyrite_gpu.h")
f32 = np.float32
IMAGE_ENTRIES = ["pyr_image_despeckle", "pyr_image_despeckle_device"]
NEW_ENTRIES = IMAGE_ENTRIES + ["pyr_session_despeckled"]
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    gpu_build.build()
    return abi.bind(C.CDLL(gpu_build.OUT))


# ------------------------------------------------------------------------------------------------------------------------ the ABI
def test_header_abi_and_library_agree(lib, tmp_path):
    header = open(HEADER).read()
    for name in NEW_ENTRIES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in abi.ENTRY_POINTS and hasattr(lib, name)
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "%s"' % HEADER, "int main(void){", 'printf("size %zu\\n", sizeof(PyrDespeckleParams));']
    for field, _ in abi.PyrDespeckleParams._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(PyrDespeckleParams, %s));' % (field, field))
    lines += ['printf("floats %.9g %.9g %.9g\\n", (double)PYR_DESPECKLE_K, (double)PYR_DESPECKLE_RELATIVE, (double)PYR_DESPECKLE_FLOOR);',
              'printf("ints %u %u %u\\n", PYR_DESPECKLE_RADIUS, PYR_DESPECKLE_MOST_RADIUS, PYR_DESPECKLE_LEAST_SAMPLES);', "return 0;}"]
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    open(src, "w").write("\n".join(lines))
    subprocess.check_call(["gcc", "-o", exe, src])
    seen = dict(line.split(None, 1) for line in subprocess.check_output([exe]).decode().splitlines())
    assert int(seen["size"]) == C.sizeof(abi.PyrDespeckleParams) == 32
    assert [name for name, _ in abi.PyrDespeckleParams._fields_] == ["radius", "k", "relative", "floor", "flags", "reserved"]
    for field, _ in abi.PyrDespeckleParams._fields_:
        assert int(seen[field]) == getattr(abi.PyrDespeckleParams, field).offset, field
    assert [f32(float(v)) for v in seen["floats"].split()] == [f32(abi.PYR_DESPECKLE_K), f32(abi.PYR_DESPECKLE_RELATIVE), f32(abi.PYR_DESPECKLE_FLOOR)] == [f32(6), f32(0.1), f32(1e-4)]
    assert [int(v) for v in seen["ints"].split()] == [abi.PYR_DESPECKLE_RADIUS, abi.PYR_DESPECKLE_MOST_RADIUS, abi.PYR_DESPECKLE_LEAST_SAMPLES] == [2, 2, 5]
    assert (R.MOST_RADIUS, R.LEAST_SAMPLES) == (2, 5)
    assert "#define PYR_ABI_VERSION 5\n" in header and abi.PYR_ABI_VERSION == 5 and lib.pyr_abi_version() == 5  # additions only


def test_the_python_defaults_are_the_header_s():
    p = develop.despeckle_params()
    assert (p.radius, f32(p.k), f32(p.relative), f32(p.floor), p.flags, list(p.reserved)) == (2, f32(6), f32(0.1), f32(1e-4), 0, [0, 0, 0])
    assert develop.despeckle_params(radius=1, k=4).radius == 1 and develop.despeckle_params(k=4).k == 4 and develop.despeckle_params(flags=2).flags == 2
    defaults = {k: v.default for k, v in inspect.signature(R.despeckle).parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(b=None, radius=2, k=6.0, relative=0.1, floor=1e-4)  # the restatement's too


# ------------------------------------------------------------------------------------------------------------------------ the argument checks
def despeckle_call(lib, entry="pyr_image_despeckle", missing=(), with_b=True, params=True, width=4, height=3, device=99, same=None, **fields):
    """One call with 4 x 3 buffers of zeros; `missing` names the pointers passed as NULL, beyond b and b_out without `with_b`;
    `same`: a pair of names given the same address. Images that are refused for their size get addresses never read."""
    names = ["a", "b", "a_out", "b_out", "removed_out", "counts_out"]
    small = width * height <= 12
    store = np.zeros(6 * 256 + 64, dtype=np.uint8)
    base = (store.ctypes.data + 31) & ~31
    at = {name: (base + k * 256) if small else ((k + 1) << 44) for k, name in enumerate(names)}
    if not with_b:
        missing = tuple(missing) + ("b", "b_out")
    if same:
        at[same[0]] = at[same[1]]
    p = develop.despeckle_params()
    for name, value in fields.items():
        if name == "reserved":
            p.reserved[value] = 1
        else:
            setattr(p, name, value)
    ptr = lambda name: None if name in missing else at[name]  # noqa: E731
    args = [ptr("a"), ptr("b"), width, height, C.byref(p) if params else None, ptr("a_out"), ptr("b_out"), ptr("removed_out"), ptr("counts_out"), device]
    if entry.endswith("_device"):
        args.append(None)
    rc = getattr(lib, entry)(*args)
    return rc, lib.pyr_last_error().decode()


REFUSED = [
    (dict(missing=("a",)), "a"), (dict(params=False), "params"), (dict(missing=("a_out",)), "a_out"),
    (dict(missing=("b",)), "b_out"), (dict(missing=("b_out",)), "b"),
    (dict(width=0), "width"), (dict(height=0), "height"),
    (dict(radius=0), "radius"), (dict(radius=3), "radius"), (dict(radius=0xFFFFFFFF), "radius"),
    (dict(k=0.0), "k"), (dict(k=-1.0), "k"), (dict(k=NAN), "k"), (dict(k=INF), "k"),
    (dict(relative=-0.5), "relative"), (dict(relative=NAN), "relative"), (dict(relative=INF), "relative"),
    (dict(floor=0.0), "floor"), (dict(floor=-1e-4), "floor"), (dict(floor=NAN), "floor"), (dict(floor=INF), "floor"),
    (dict(flags=1), "flags"), (dict(flags=0x80000000), "flags"),
    (dict(reserved=0), "reserved"), (dict(reserved=1), "reserved"), (dict(reserved=2), "reserved"),
    (dict(same=("a_out", "a")), "a_out"), (dict(same=("b_out", "b")), "b_out"), (dict(same=("a_out", "b")), "a_out"), (dict(same=("b_out", "a")), "b_out"),
    (dict(same=("removed_out", "a")), "removed_out"), (dict(same=("b_out", "a_out")), "a_out"), (dict(same=("removed_out", "b_out")), "b_out"),
]


def names_in(message):
    return message.replace("params->", " ").replace("_device", "").replace(":", " ").replace(",", " ").split()


@pytest.mark.parametrize("entry", IMAGE_ENTRIES)
@pytest.mark.parametrize("change,name", REFUSED)
def test_the_despeckle_refuses_bad_arguments_by_name_before_a_device_is_looked_for(change, name, entry, lib):
    rc, message = despeckle_call(lib, entry=entry, **change)  # no device 99: the argument is still what is reported
    assert rc == abi.PYR_ERR_INVALID_ARGUMENT
    assert name in names_in(message), message


@pytest.mark.parametrize("entry", IMAGE_ENTRIES)
def test_the_order_of_the_refusals_then_the_device(entry, lib):
    """Nulls, then half a pair, then the size rules, then the parameters, then the overlaps; valid arguments end in PYR_ERR_DEVICE."""
    assert "null argument" in despeckle_call(lib, entry=entry, missing=("a", "b"), width=0, radius=0)[1]
    assert "both null or both given" in despeckle_call(lib, entry=entry, missing=("b",), width=0, radius=0)[1]
    assert "width" in despeckle_call(lib, entry=entry, width=0, radius=0)[1]
    rc, message = despeckle_call(lib, entry=entry, width=65536, height=65536, radius=0)  # 2^32 pixels before a parameter
    assert rc == abi.PYR_ERR_UNSUPPORTED and "2^32" in message
    assert despeckle_call(lib, entry=entry, width=65535, height=65537, radius=0)[1].startswith("params->radius")  # 2^32 - 1 pixels pass
    assert despeckle_call(lib, entry=entry, radius=0, same=("a_out", "a"))[1].startswith("params->radius")  # a parameter before an overlap
    assert "overlaps" in despeckle_call(lib, entry=entry, same=("a_out", "a"))[1]
    assert despeckle_call(lib, entry=entry)[0] == abi.PYR_ERR_DEVICE
    assert despeckle_call(lib, entry=entry, with_b=False)[0] == abi.PYR_ERR_DEVICE
    assert despeckle_call(lib, entry=entry, missing=("removed_out", "counts_out"))[0] == abi.PYR_ERR_DEVICE  # the reports are optional
    assert despeckle_call(lib, entry=entry, radius=1, k=1e-30, relative=0.0, floor=1e-38)[0] == abi.PYR_ERR_DEVICE  # the edges are inside
    assert despeckle_call(lib, entry=entry, width=1, height=1)[0] == abi.PYR_ERR_DEVICE
    if lib.pyr_device_count() <= 0:  # valid arguments where there is no GPU
        assert despeckle_call(lib, entry=entry, device=0)[0] == abi.PYR_ERR_DEVICE


def test_the_session_entry_names_what_is_missing(lib):
    p, d, out = develop.despeckle_params(), abi.PyrDevelopParams(), np.zeros(3, dtype=f32)
    session = C.c_void_p(1)  # never read: every check below comes before the session is looked at
    call = lambda s, dev, sp, o: lib.pyr_session_despeckled(s, dev, sp, None, None, o, None, None, None)  # noqa: E731
    for args, name in (((None, C.byref(d), C.byref(p), out.ctypes.data), "session"), ((session, None, C.byref(p), out.ctypes.data), "develop_params"),
                       ((session, C.byref(d), C.byref(p), None), "out"), ((session, C.byref(d), None, out.ctypes.data), "despeckle_params")):
        assert call(*args) == abi.PYR_ERR_INVALID_ARGUMENT
        assert lib.pyr_last_error().decode().split()[-1] == name
    for field, value in (("radius", 3), ("k", 0.0), ("relative", NAN), ("floor", 0.0), ("flags", 4)):
        p = develop.despeckle_params()
        setattr(p, field, value)
        assert call(session, C.byref(d), C.byref(p), out.ctypes.data) == abi.PYR_ERR_INVALID_ARGUMENT
        assert lib.pyr_last_error().decode().startswith("despeckle_params->" + field)
    p = develop.despeckle_params()
    p.reserved[2] = 7
    assert call(session, C.byref(d), C.byref(p), out.ctypes.data) == abi.PYR_ERR_INVALID_ARGUMENT and lib.pyr_last_error().decode().startswith("despeckle_params->reserved")


def test_the_python_wrapper_checks_its_images(lib):
    a = np.zeros((3, 4, 3), dtype=f32)
    with pytest.raises(AssertionError):
        develop.despeckle(np.zeros((3, 4), dtype=f32), device=99)
    with pytest.raises(AssertionError):
        develop.despeckle(a, np.zeros((4, 3, 3), dtype=f32), device=99)  # the halves have one size
    with pytest.raises(TypeError):
        develop.despeckle(a, a.copy(), strength=0.5, device=99)
    for params, name in ((dict(radius=3), "radius"), (dict(k=0), "k"), (dict(relative=-1), "relative"), (dict(floor=0), "floor"), (dict(flags=1), "flags")):
        with pytest.raises(Exception) as refused:
            develop.despeckle(a, a.copy(), device=99, **params)
        assert "params->" + name in str(refused.value)
    for b in (a.copy(), None):
        with pytest.raises(Exception) as refused:  # good arguments reach the library, which finds no device 99
            develop.despeckle(a, b, radius=1, k=4.0, device=99)
        assert not isinstance(refused.value, (AssertionError, ValueError, TypeError))


# ------------------------------------------------------------------------------------------------------------------------ the C++ wrappers
def test_the_cpp_wrappers(lib, tmp_path):
    """pyrite::despeckle, despeckle_params, despeckle_flag_problem and despeckle_from_flags from a stand-alone program
    (tests/despeckle_driver.cpp) linked against libpyrite_host.so: the ProjectError for a buffer of the wrong size, the GpuError and
    its status for a parameter out of range, and with good arguments PYR_ERR_DEVICE here -- or, where there is a GPU, a constant
    image that comes back bit for bit and a planted pixel that lands on the limit."""
    exe = str(tmp_path / "despeckle_driver")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "despeckle_driver.cpp"), "-L" + gpu_build.HOST_DIR, "-lpyrite_host", "-L" + gpu_build.CSRC, "-lpyrite_gpu",
                           "-Wl,-rpath," + gpu_build.HOST_DIR, "-Wl,-rpath," + gpu_build.CSRC])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr[-2000:]
    assert run.stdout.split()[0] == "ok"


# ------------------------------------------------------------------------------------------------------------------------ the flags
PROJECT = os.path.join(ROOT, "tests", "golden", "projects", "gallery.lua")
EVEN = "--despeckle needs an even number of samples per pixel: the two half films must be equal"
BAD_FLAGS = [
    (["--despeckle-radius", "2"], "--despeckle-radius needs --despeckle"),
    (["--despeckle", "0"], "--despeckle must be a finite number above 0"),
    (["--despeckle", "-3"], "--despeckle must be a finite number above 0"),
    (["--despeckle", "nan"], "--despeckle must be a finite number above 0"),
    (["--despeckle", "inf"], "--despeckle must be a finite number above 0"),
    (["--despeckle", "six"], "--despeckle must be a finite number above 0"),
    (["--despeckle", "--despeckle-radius", "0"], "--despeckle-radius must be 1 to 2"),
    (["--despeckle", "4", "--despeckle-radius", "3"], "--despeckle-radius must be 1 to 2"),
    (["--despeckle", "--spp", "5"], EVEN),  # an odd budget, as --denoise refuses it, before anything renders
    (["--despeckle", "--spp", "12", "--pass-samples", "4"], "--despeckle needs an even number of equal passes: the samples per pixel must be a multiple of twice --pass-samples"),
]


def test_flag_rules():
    assert develop.despeckle_flag_problem(None, None) is None and develop.despeckle_from_flags(None, None) is None
    assert develop.despeckle_flag_problem("6.0", None) is None and develop.despeckle_flag_problem(4, 1, 8, 2) is None
    assert develop.despeckle_flag_problem(None, 2) == BAD_FLAGS[0][1] and develop.despeckle_flag_problem("0", None) == BAD_FLAGS[1][1]
    assert develop.despeckle_flag_problem("6", 3) == BAD_FLAGS[6][1] and develop.despeckle_flag_problem("6", None, 5) == EVEN
    assert develop.despeckle_from_flags("6.0", None) == dict(k=6.0) and develop.despeckle_from_flags("4", 1) == dict(k=4.0, radius=1)


@pytest.mark.parametrize("flags,message", BAD_FLAGS, ids=lambda v: "_".join(v).strip("-") if isinstance(v, list) else None)
def test_both_front_ends_reject_the_same_flags_in_the_same_words(flags, message, lib):
    py = subprocess.run([sys.executable, "-m", "pyrite_amd", PROJECT] + flags, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
    cpp = subprocess.run([gpu_build.HOST_TOOL, "render-project", PROJECT, "-", "1", os.devnull] + flags, cwd=ROOT, capture_output=True, text=True)
    assert py.returncode == 2 and cpp.returncode == 2, py.stderr + cpp.stderr
    assert py.stderr.strip() == cpp.stderr.strip() == "error: " + message
    assert "Rendering" not in py.stdout + cpp.stdout and "The scene contains" not in py.stdout + cpp.stdout  # before anything renders


def test_both_front_ends_parse_the_flags(lib, tmp_path):
    """Well-formed flags get past the parser: what stops the run here is the missing GPU (or nothing, on a GPU box)."""
    for flags in (["--despeckle"], ["--despeckle", "4.5", "--despeckle-radius", "1", "--denoise", "--denoise-radius", "2", "--glare", "--tone", "reinhard"]):
        flags = flags + ["--spp", "2", "--size", "16x16"]
        py = subprocess.run([sys.executable, "-m", "pyrite_amd", PROJECT, "-o", str(tmp_path / "a.png")] + flags, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                            capture_output=True, text=True)
        cpp = subprocess.run([gpu_build.HOST_TOOL, "render-project", PROJECT, "-", "1", str(tmp_path / "b.png")] + flags, cwd=ROOT, capture_output=True, text=True)
        for run in (py, cpp):
            assert "unrecognized" not in run.stderr and "unknown flag" not in run.stderr and "must" not in run.stderr and "needs" not in run.stderr, run.stderr
            assert run.returncode == 0 or "HIP device" in run.stderr, run.stderr


# ------------------------------------------------------------------------------------------------------------------------ the addresses
def test_the_tile_addressing_stays_in_range_under_the_sanitizers(tmp_path):
    """tests/probes/despeckle_address_check.cpp: a program of its own with the kernel's addressing function, run as a child process;
    nothing is loaded into this interpreter."""
    exe = tmp_path / "despeckle_address_check"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-o", str(exe), os.path.join(ROOT, "tests", "probes", "despeckle_address_check.cpp")])
    run = subprocess.run([str(exe)], capture_output=True, text=True)  # the runtimes are linked statically: the environment stays as it is
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok: ")


# ------------------------------------------------------------------------------------------------------------------------ the kernel's resources
def test_the_kernel_keeps_its_values_in_registers(tmp_path):
    """kernels/despeckle.hip cross-compiled for gfx950 as tests/test_kernel_isa.py obtains its listing: the private segment of both
    builds of the kernel is 0 -- the 16 or 48 gathered values, the sorting network and the pick of the median stay in registers --
    and the compiler's other figures are printed. Only the metadata is read."""
    flags = [f for f in gpu_build.FLAGS if f not in ("-shared", "-fPIC")]
    out = tmp_path / "despeckle.s"
    subprocess.check_call([gpu_build.HIPCC] + flags + ["--cuda-device-only", "-S", "kernels/despeckle.hip", "-o", str(out)], cwd=gpu_build.CSRC, stderr=subprocess.DEVNULL)
    text = out.read_text()
    kernels = re.findall(r"^\s*\.amdhsa_kernel (\S*despeckle_kernel\S*)", text, re.M)
    assert len(kernels) == 2, kernels  # radius 1 and radius 2
    for name in kernels:
        meta = text[text.index(".amdhsa_kernel " + name):]
        meta = meta[:meta.index(".end_amdhsa_kernel")]
        figure = lambda key: int(re.search(r"\.amdhsa_%s (\d+)" % key, meta).group(1))  # noqa: E731
        scratch, vgprs, sgprs, lds = figure("private_segment_fixed_size"), figure("next_free_vgpr"), figure("next_free_sgpr"), figure("group_segment_fixed_size")
        print("%s: %d VGPRs, %d SGPRs, %d B of scratch, %d B of LDS" % (name, vgprs, sgprs, scratch, lds))
        assert scratch == 0, "%s keeps %d B in scratch: an index into the register array is no longer static" % (name, scratch)
        assert lds in (18 * 48 * 8 + 8, 20 * 48 * 8 + 8) and vgprs <= 128  # the tile and the two words of the tally


# ------------------------------------------------------------------------------------------------------------------------ the rule itself
def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=f32).view(np.uint32), np.asarray(b, dtype=f32).view(np.uint32))


HEIGHT, WIDTH, EDGE = 40, 48, 24
PLANTED = [(0, 0), (HEIGHT - 1, WIDTH - 1), (10, EDGE - 1), (10, EDGE), (20, 7), (30, 40), (5, 30)]  # two corners, two neighbours across the edge
BOTH = (25, 12)
SEEDS = {0.3: 4, 0.6: 3}  # chosen so that the restatement stays within the 2 % cap below; what is seen is printed


def edge_scene(sigma, seed):
    """A 40 x 48 image with a 1 : 20 vertical edge under multiplicative log-normal noise, independent per half, one factor a pixel;
    seven pixels times 200 in alternating halves and one pixel at 500 in both. Returns (clean, a, b, a and b before the planting)."""
    rng = np.random.default_rng(seed)
    clean = np.ones((HEIGHT, WIDTH, 3), dtype=f32)
    clean[:, EDGE:] = 20
    clean *= np.array([0.9, 1.0, 0.8], dtype=f32)
    halves = [(clean * np.exp(rng.normal(0, sigma, (HEIGHT, WIDTH, 1)))).astype(f32) for _ in range(2)]
    for half in halves:
        half[BOTH] = 500
    pure = [half.copy() for half in halves]
    for i, at in enumerate(PLANTED):
        halves[i % 2][at] *= f32(200)
    return clean, halves[0], halves[1], pure


@pytest.fixture(scope="module")
def cleaned():
    """sigma -> (the scene, what the restatement makes of it): computed once, shared, never written to."""
    return {sigma: (edge_scene(sigma, seed), R.despeckle(*edge_scene(sigma, seed)[1:3])) for sigma, seed in SEEDS.items()}


@pytest.mark.parametrize("sigma", sorted(SEEDS))
def test_planted_fireflies_go_and_what_both_halves_saw_stays(sigma, cleaned):
    (clean, a, b, pure), (a_out, b_out, removed, counts) = cleaned[sigma]
    for i, at in enumerate(PLANTED):
        before, after = (a, b)[i % 2], (a_out, b_out)[i % 2]
        assert not same_bits(after[at], before[at]), "the planted pixel %r was kept" % (at,)
        assert R.luminance(after[at]) < R.luminance(before[at]) / 10
        assert same_bits((b_out, a_out)[i % 2][at], (b, a)[i % 2][at]), "the other half changed at %r" % (at,)
        ratio = after[at] / before[at]
        assert np.allclose(ratio, ratio[0], rtol=1e-6), "the hue is kept"
    assert same_bits(a_out[BOTH], a[BOTH]) and same_bits(b_out[BOTH], b[BOTH]), "the pixel bright in both halves keeps its bits"
    changed = (a_out.view(np.uint32) != a.view(np.uint32)).any(axis=-1) | (b_out.view(np.uint32) != b.view(np.uint32)).any(axis=-1)
    others = int(changed.sum()) - len(PLANTED)
    share = others / (HEIGHT * WIDTH - len(PLANTED) - 1)
    print("sigma %.1f seed %d: %d of 7 planted clamped, %d other pixels changed (%.2f %%), counts %r" % (sigma, SEEDS[sigma], len(PLANTED), others, 100 * share, counts))
    assert share <= 0.02
    assert counts == (int((a_out.view(np.uint32) != a.view(np.uint32)).any(axis=-1).sum()), int((b_out.view(np.uint32) != b.view(np.uint32)).any(axis=-1).sum()))
    lost = ((a - a_out) + (b - b_out)) * f32(0.5)
    assert same_bits(removed, lost), "removed is what the mean lost"
    assert (removed != 0).any(axis=-1).sum() == changed.sum()


def test_the_error_of_the_mean_falls_tenfold(cleaned):
    (clean, a, b, pure), (a_out, b_out, _, _) = cleaned[0.3]
    keep = np.ones((HEIGHT, WIDTH), dtype=bool)
    keep[BOTH] = False  # the lamp both halves saw is no part of the clean image
    rmse = lambda image: float(np.sqrt(((((image - clean) / clean)[keep]).astype(np.float64) ** 2).mean()))  # noqa: E731
    before, after, never = rmse((a + b) * f32(0.5)), rmse((a_out + b_out) * f32(0.5)), rmse((pure[0] + pure[1]) * f32(0.5))
    print("sigma 0.3: relative RMSE of the mean before %.3f, after %.3f, never contaminated %.3f" % (before, after, never))
    assert after * 10 <= before


@pytest.mark.parametrize("sigma", sorted(SEEDS))
def test_one_image_alone_clamps_more(sigma, cleaned):
    (clean, a, b, _), (_, _, _, counts) = cleaned[sigma]
    a_out, none, removed, alone = R.despeckle(a)
    assert none is None and alone[1] == 0
    print("sigma %.1f: %d pixels of a clamped alone, %d with b" % (sigma, alone[0], counts[0]))
    assert alone[0] > counts[0], "without the other half more is clamped: the price of the one-image form"
    assert same_bits(removed, a - a_out)
    changed = (a_out.view(np.uint32) != a.view(np.uint32)).any(axis=-1)
    assert changed[BOTH], "what both halves saw is a firefly to one image alone"


def test_a_constant_image_comes_back_bit_for_bit():
    for value in (3.7, 0.0, 1e-30, 1e30):
        image = np.full((9, 11, 3), value, dtype=f32)
        for b in (image.copy(), None):
            for radius in (1, 2):
                a_out, b_out, removed, counts = R.despeckle(image, b, radius=radius)
                assert same_bits(a_out, image) and counts == (0, 0) and not removed.any()
                assert b is None or same_bits(b_out, b)


def test_a_flat_zero_block_takes_the_floor():
    a, b = np.zeros((9, 9, 3), dtype=f32), np.zeros((9, 9, 3), dtype=f32)
    a[4, 4] = 5e-4  # below six floors: kept
    a_out, b_out, _, counts = R.despeckle(a, b)
    assert same_bits(a_out, a) and counts == (0, 0)
    a[4, 4] = 7e-4  # above: its luminance lands on k * floor
    a_out, b_out, removed, counts = R.despeckle(a, b)
    assert counts == (1, 0) and same_bits(b_out, b)
    assert abs(float(R.luminance(a_out[4, 4])) - 6e-4) <= 1e-9
    assert R.despeckle(a, b, floor=2e-4)[3] == (0, 0)  # the floor is what decides
    changed = (a_out != a).any(axis=-1)
    assert changed.sum() == 1 and changed[4, 4]


def test_what_is_not_finite_keeps_its_bits_and_clamps_nobody():
    rng = np.random.default_rng(5)
    a, b = (rng.uniform(0.5, 2.0, (12, 12, 3)).astype(f32) for _ in range(2))
    plain = R.despeckle(a, b)
    assert plain[3] == (0, 0)
    bad = [((3, 3), (np.nan, 1, 1)), ((3, 8), (np.inf, 1, 1)), ((8, 3), (1, -np.inf, 1)), ((8, 8), (np.inf, -np.inf, 1))]
    for at, value in bad:
        a[at] = value
    a.view(np.uint32)[3, 3, 0] = 0xFFC12345  # a NaN with a sign and a payload
    a_out, b_out, removed, counts = R.despeckle(a, b)
    assert same_bits(a_out, a) and same_bits(b_out, b) and counts == (0, 0)
    assert not removed.any() and np.isfinite(removed).all()
    for radius in (1, 2):
        alone = R.despeckle(a, radius=radius)[0]  # one image may clamp a pixel of the noise; what is not finite it keeps
        assert all(same_bits(alone[at], a[at]) for at, _ in bad)
    a[5, 5] *= f32(300)  # a firefly beside them is still found: they are no samples
    assert R.despeckle(a, b)[3] == (1, 0)


def test_fewer_than_five_samples_touch_nothing():
    a, b = np.array([[[1, 1, 1], [1000, 1000, 1000]]], dtype=f32), np.ones((1, 2, 3), dtype=f32)  # 2 x 1: n = 2
    a_out, b_out, removed, counts = R.despeckle(a, b)
    assert same_bits(a_out, a) and same_bits(b_out, b) and counts == (0, 0) and not removed.any()
    one = np.full((1, 1, 3), 1000, dtype=f32)
    assert same_bits(R.despeckle(one, one.copy())[0], one)
    a = np.ones((1, 3, 3), dtype=f32)  # 3 x 1: the middle pixel has 2 + 2 = 4 samples, with one half 2
    a[0, 1] = 1000
    assert R.despeckle(a, np.ones((1, 3, 3), dtype=f32), radius=1)[3] == (0, 0)
    a = np.ones((1, 5, 3), dtype=f32)  # 5 x 1 at radius 2: 4 + 4 = 8 samples with both halves, 4 with one
    a[0, 2] = 1000
    assert R.despeckle(a, np.ones((1, 5, 3), dtype=f32))[3] == (1, 0) and R.despeckle(a)[3] == (0, 0)


def test_the_medians_are_the_lower_ones():
    """Six samples around the second pixel of a 4 x 1 image, 1, 2, 9 in one half and 1, 4, 9 in the other: the lower median is
    element (6-1)/2 = 2 of 1, 1, 2, 4, 9, 9, which is 2 where an averaging median gives 3. The deviations 1, 1, 0, 2, 7, 7 sort to
    0, 1, 1, 2, 7, 7: s = 1, element 2 again. With relative 0 and a tiny floor the limit is m + k * (s * 1.4826f)."""
    a, b = np.zeros((1, 4, 3), dtype=f32), np.zeros((1, 4, 3), dtype=f32)
    grey = lambda y: np.full(3, y, dtype=f32)  # noqa: E731
    a[0], b[0] = [grey(1), grey(100), grey(2), grey(9)], [grey(1), grey(0), grey(4), grey(9)]
    limit, n = R.limits([R.luminance(a), R.luminance(b)], 2, 6.0, 0.0, 1e-30)
    assert n[0, 1] == 6
    y = lambda v: R.luminance(grey(v))  # noqa: E731
    m, s = y(2), abs(f32(y(1) - y(2)))
    assert limit[0, 1] == f32(m + f32(f32(6.0) * f32(s * f32(1.4826))))
