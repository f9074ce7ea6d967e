"""The first-hit feature pass on the GPU (include/pyrite_gpu.h "first-hit feature images") against an
expectation composed on the CPU from the oracle's entry points: rays from oracle_to_view_area and oracle_ray_towards with the
aperture set to 0, hits, surface data and programs from OracleScene.intersect / surface_data / run_program, and the header's
formulas applied in numpy float32 in the stated order. Shape, material and coverage must agree in every pixel; depth, normal and
albedo within 1e-5 (DESIGN.md section 4's figure for GPU against oracle). The observed maxima are printed, one line per case
("features <case> grid G bins B: ..."), for profiles/r07_features_parity.txt."""
import ctypes as C
import functools
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import oracle
from pyrite_amd import abi, lua_project, scenes
from pyrite_amd import build as gpu_build
from pyrite_amd._lib import check, lib
from pyrite_amd.develop import develop
from pyrite_amd.features import RECORD, Features, encode_depth, encode_normal
from pyrite_amd.renderer import Camera, Renderer, World

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROJECTS = os.path.join(ROOT, "tests", "golden", "projects")
TOL = 1e-5  # DESIGN.md section 4; tests/test_gpu_session.py TOL
f32 = np.float32


def rel_l2(film, reference):  # tests/test_gpu_session.py rel_l2, restated
    a, b = film.develop(), reference.develop()
    return (np.sqrt(((a - b) ** 2).sum(-1)) / (np.sqrt((b ** 2).sum(-1)) + 1e-6)).reshape(-1)


def assert_same_film(film, reference, what):  # tests/test_gpu_session.py assert_same_film, restated
    e = rel_l2(film, reference)
    worst = float(e.max()) if e.size else 0.0
    print("%s: relL2 max %.3g, weights equal: %s" % (what, worst, np.array_equal(film.grains[..., 1], reference.grains[..., 1])))
    assert np.array_equal(film.grains[..., 1], reference.grains[..., 1]), what + ": film weights differ"
    assert worst <= TOL, what
    assert not np.isnan(film.grains).any()


def c2_case():
    world, cam, r, film = scenes.build(scenes.c2_cornell(64, 64, 16), seed=5)
    return world, cam, r, (64, 64)


def c3_case():  # tests/test_gpu_session.py c3_case
    project = scenes.c3_mesh_in_box(width=64, height=36, pixel_samples=16)
    world = World(scenes.c3_flat(segments=96, sides=48))
    return world, Camera.from_project(project["camera"]), Renderer.from_project(project["renderer"], seed=6), (64, 36)


def textures_case():
    world, cam, r, film = scenes.build(scenes.textures_example(72, 48, 16), seed=5)
    return world, cam, r, (72, 48)


def lamps_case():
    world, cam, r, film = scenes.build(scenes.lamps_example(96, 64, 16), seed=5)
    return world, cam, r, (96, 64)


def wide_case():
    cwd = os.getcwd()
    os.chdir(PROJECTS)
    try:
        world, cam, r, film = scenes.build(scenes.wide_program_project(False), seed=1)
    finally:
        os.chdir(cwd)
    return world, cam, r, (film.width, film.height)


CASES = {"c2_cornell": c2_case, "c3_shaped": c3_case, "textures_example": textures_case, "lamps_example": lamps_case, "wide_program": wide_case}


@functools.lru_cache(maxsize=None)
def case(name):
    """(world, camera, renderer, (width, height), OracleScene), built once and shared: nothing here changes them."""
    world, cam, r, size = CASES[name]()
    return world, cam, r, size, oracle.OracleScene(world)


def camera_rays(cam, width, height, grid):
    """float32 [height, width, grid*grid, 6]: section 1's rays from the oracle's to_view_area and ray_towards, aperture 0."""
    L = oracle.lib()
    pinhole = abi.PyrCamera.from_buffer_copy(cam.c)
    pinhole.aperture = 0.0
    rays = np.zeros((height, width, grid * grid, 6), dtype=f32)
    area, ray, state = (C.c_float * 4)(), oracle.F6(), oracle.U4(1, 2, 3, 4)
    for y in range(height):
        for x in range(width):
            L.oracle_to_view_area(x, y, 1, 1, width, height, area)
            fx0, fy0, sx, sy = (f32(v) for v in area)
            for j in range(grid * grid):
                jy, jx = divmod(j, grid)
                fx, fy = f32(f32(jx) + f32(0.5)) / f32(grid), f32(f32(jy) + f32(0.5)) / f32(grid)
                L.oracle_ray_towards(C.byref(pinhole), state, f32(fx0 + f32(sx * fx)), f32(fy0 + f32(sy * fy)), ray)
                rays[y, x, j] = ray[:]
    assert list(state) == [1, 2, 3, 4]  # no random number was drawn
    return rays


def material_of(desc, shape):
    kind, index = int(shape) >> 30, int(shape) & 0x3FFFFFFF
    return int({abi.SHAPE_TRIANGLE: desc.tri_material, abi.SHAPE_SPHERE: desc.sphere_material, abi.SHAPE_PLANE: desc.plane_material}[kind][index])


@functools.lru_cache(maxsize=None)
def first_hits(name, grid):
    """Per sub-sample: rays, the oracle's hits, shading normal, texture coordinates, material -- computed once per (case, grid)."""
    world, cam, r, (width, height), scene = case(name)
    span = r.spectrum_span
    normal_wl = f32(f32(span[0]) + f32(f32(span[1] - span[0]) * f32(0.5)))
    rays = camera_rays(cam, width, height, grid)
    flat = rays.reshape(-1, 6)
    hits, _ = scene.intersect(flat)
    n = len(flat)
    normal, texture, material = np.zeros((n, 3), dtype=f32), np.zeros((n, 2), dtype=f32), np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    for i in np.nonzero(hits["shape"] != abi.HIT_NONE)[0]:
        _, t, _, shading = scene.surface_data(flat[i], wavelength=float(normal_wl))
        normal[i], texture[i], material[i] = shading, t, material_of(world.desc, hits["shape"][i])
    shape = (height, width, grid * grid)
    return rays, hits.reshape(shape), normal.reshape(shape + (3,)), texture.reshape(shape + (2,)), material.reshape(shape)


def program_reads_the_hit(desc, program):
    p = desc.programs[program]
    if p.kind == abi.PROGRAM_CONSTANT:
        return False
    deps = 0
    for k in range(p.num_instrs):
        deps |= desc.instrs[p.first_instr + k].deps
    return bool(deps & (abi.DEP_NORMAL | abi.DEP_INCIDENT | abi.DEP_TEXTURE))


@functools.lru_cache(maxsize=None)
def expected(name, grid, bins):
    """(records [h, w] of RECORD, albedo grains [h, w, bins, 2]) by section 1's formulas in float32."""
    world, cam, r, (width, height), scene = case(name)
    desc = world.desc
    rays, hits, normal, texture, material = first_hits(name, grid)
    sub = grid * grid
    hit = hits["shape"] != abi.HIT_NONE
    rec = np.zeros((height, width), dtype=RECORD)
    nsum, dsum, count = np.zeros((height, width, 3), dtype=f32), np.zeros((height, width), dtype=f32), np.zeros((height, width), dtype=f32)
    for j in range(sub):  # sums in sub-sample order
        nsum = np.where(hit[..., j, None], nsum + normal[..., j, :], nsum)
        dsum = np.where(hit[..., j], dsum + hits["distance"][..., j], dsum)
        count = count + hit[..., j].astype(f32)
    some = count > 0
    with np.errstate(all="ignore"):
        rec["normal"] = np.where(some[..., None], nsum / count[..., None], f32(0))
        rec["depth"] = np.where(some, dsum / count, f32(0))
    rec["coverage"] = count / f32(sub)
    rec["shape"], rec["material"] = hits["shape"][..., sub // 2], material[..., sub // 2]
    # albedo
    start, width_wl = f32(r.spectrum_span[0]), f32(r.spectrum_span[1] - r.spectrum_span[0])
    bin_width = f32(width_wl / f32(bins))
    wavelengths = [f32(start + f32(f32(f32(b) + f32(0.5)) * bin_width)) for b in range(bins)]
    reads_hit = {}
    cache = {}

    def run(program, wl, n, d, t):
        if program not in reads_hit:
            reads_hit[program] = program_reads_the_hit(desc, program)
        if not reads_hit[program]:  # a function of the wavelength alone: one evaluation serves every hit
            key = (program, float(wl))
            if key not in cache:
                cache[key] = f32(scene.run_program(program, float(wl), n, d, t)[0])
            return cache[key]
        return f32(scene.run_program(program, float(wl), n, d, t)[0])

    def albedo_of(m, n, d, t):  # a of one sub-sample, per bin: components in list order, one division by N
        comps = [desc.components[m.first_component + c] for c in range(m.num_components)]
        out = np.zeros(bins, dtype=f32)
        for b, wl in enumerate(wavelengths):
            total = f32(0)
            for c in comps:
                if c.bsdf == abi.BSDF_EMISSIVE:
                    continue
                prob = f32(c.selection_compensation)
                if c.probability_program >= 0:
                    prob = f32(run(c.probability_program, wl, n, d, t) * prob)
                total = f32(total + f32(prob * run(c.color_program, wl, n, d, t)))
            out[b] = f32(total / f32(m.num_components))
        return out

    a = np.zeros((height, width, sub, bins), dtype=f32)  # 0 on a miss
    for index in np.unique(material[hit]):
        m = desc.materials[int(index)]
        if m.num_components == 0:
            continue
        programs = [p for c in range(m.num_components) for p in (desc.components[m.first_component + c].color_program, desc.components[m.first_component + c].probability_program) if p >= 0]
        where = hit & (material == index)
        if not any(program_reads_the_hit(desc, p) for p in programs):  # the same spectrum at every hit of this material
            a[where] = albedo_of(m, (0, 0, 1), (0, 0, -1), (0, 0))
        else:
            for y, x, j in zip(*np.nonzero(where)):
                a[y, x, j] = albedo_of(m, normal[y, x, j], rays[y, x, j, 3:], texture[y, x, j])
    grains = np.zeros((height, width, bins, 2), dtype=f32)
    grains[..., 1] = f32(sub)
    for j in range(sub):  # acc += a in sub-sample order
        grains[..., 0] = grains[..., 0] + a[:, :, j, :]
    return rec, grains


def gpu_features(name, grid, bins):
    world, cam, r, (width, height), _ = case(name)
    return r.features((width, height), cam, world, grid=grid, albedo_bins=bins)


def albedo_error(grains, reference):
    a, b = Features(1, 1).albedo, Features(1, 1).albedo
    a.grains, b.grains = grains, reference
    return rel_l2(a, b)


@pytest.mark.parametrize("bins", [5, 16])
@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("name", sorted(CASES))
def test_features_match_the_expectation(name, grid, bins, gpu_lib):
    world, cam, r, (width, height), _ = case(name)
    if name == "wide_program":
        assert r.program_info(world)["wide"] == 1
    rec, grains = expected(name, grid, bins)
    got = gpu_features(name, grid, bins)
    # hit ids: every pixel, no tolerance
    for field in ("shape", "material", "coverage"):
        differs = np.argwhere(got.records[field] != rec[field])
        assert len(differs) == 0, "%s differs in %d pixels, first (y, x) = %s: GPU %r, expected %r" % (
            field, len(differs), differs[0], got.records[field][tuple(differs[0])], rec[field][tuple(differs[0])])
    assert not got.records["reserved"].any()
    # the pass's implied hits are World::intersect's, the GPU's own, on the oracle's rays
    rays, hits, _, _, _ = first_hits(name, grid)
    own, _, _ = world.intersect(rays.reshape(-1, 6))
    own = own.reshape(hits.shape)
    assert np.array_equal(own["shape"], hits["shape"]), "pyr_scene_intersect and the oracle disagree on %d rays" % int((own["shape"] != hits["shape"]).sum())
    assert np.array_equal(got.shape, own["shape"][..., grid * grid // 2])
    assert np.array_equal(got.coverage, (own["shape"] != abi.HIT_NONE).sum(-1).astype(f32) / f32(grid * grid))
    # depth and normal
    depth_error = np.abs(got.depth - rec["depth"]) / np.maximum(np.abs(rec["depth"]), f32(1e-30))
    normal_error = np.abs(got.normal - rec["normal"])
    depth_worst, normal_worst = float(depth_error.max()), float(normal_error.max())
    # albedo
    assert np.array_equal(got.albedo.grains[..., 1], np.full((height, width, bins), grid * grid, dtype=f32)), "albedo weights are not grid^2 everywhere"
    e = albedo_error(got.albedo.grains, grains)
    print("features %s grid %d bins %d: depth max rel %.3g, normal max abs %.3g, albedo relL2 max %.3g; bit-equal: records %s, albedo %s; coverage %.3f" % (
        name, grid, bins, depth_worst, normal_worst, float(e.max()), got.records.tobytes() == rec.tobytes(), np.array_equal(got.albedo.grains, grains), float(rec["coverage"].mean())))
    assert depth_worst <= TOL and normal_worst <= TOL
    assert float(e.max()) <= TOL
    assert not np.isnan(got.albedo.grains).any() and not np.isnan(got.normal).any() and not np.isnan(got.depth).any()
    assert (np.abs(got.normal) <= 1 + TOL).all()
    if name == "lamps_example":
        assert (rec["coverage"] == 0).any() and (rec["coverage"] == 1).any()  # sky pixels miss


def raw_features(world, cam, size, grid, bins, albedo="zero", pixels="zero", fill=0.0):
    """pyr_render_features on buffers of our own: returns (albedo array or None, record array or None)."""
    width, height = size
    desc, fp = abi.PyrFilmDesc(width, height, 64, 380.0, 400.0), abi.PyrFeatureParams(grid, bins)
    a = np.full((height, width, bins, 2), fill, dtype=f32) if albedo is not None else None
    p = np.zeros((height, width), dtype=RECORD) if pixels is not None else None
    check(lib().pyr_render_features(world.scene(0), C.byref(cam.c), C.byref(desc), C.byref(fp), a.ctypes.data if a is not None else None, p.ctypes.data if p is not None else None))
    return a, p


def test_the_pass_adds_is_deterministic_and_takes_null_outputs(gpu_lib):
    world, cam, r, size, _ = case("textures_example")
    a1, p1 = raw_features(world, cam, size, 3, 5)
    a2, p2 = raw_features(world, cam, size, 3, 5)
    assert a1.tobytes() == a2.tobytes() and p1.tobytes() == p2.tobytes(), "two calls into zeroed buffers differ"
    # a second call into the same buffer: weights double exactly, accs double up to the order of the nine float additions
    width, height = size
    desc, fp = abi.PyrFilmDesc(width, height, 64, 380.0, 400.0), abi.PyrFeatureParams(3, 5)
    twice = a1.copy()
    check(lib().pyr_render_features(world.scene(0), C.byref(cam.c), C.byref(desc), C.byref(fp), twice.ctypes.data, None))
    assert np.array_equal(twice[..., 1], 2 * a1[..., 1])
    assert float(albedo_error(twice, a1).max()) <= TOL  # 2 acc / 2 weight against acc / weight
    one, _ = raw_features(world, cam, size, 1, 5)
    one_twice = one.copy()
    fp1 = abi.PyrFeatureParams(1, 5)
    check(lib().pyr_render_features(world.scene(0), C.byref(cam.c), C.byref(desc), C.byref(fp1), one_twice.ctypes.data, None))
    assert np.array_equal(one_twice, 2 * one)  # one sub-sample: one addition, exact
    # each output may be NULL, and the other is what it is without
    only_a, none_p = raw_features(world, cam, size, 3, 5, pixels=None)
    none_a, only_p = raw_features(world, cam, size, 3, 5, albedo=None)
    assert none_p is None and none_a is None and only_a.tobytes() == a1.tobytes() and only_p.tobytes() == p1.tobytes()
    fp0 = abi.PyrFeatureParams(3, 0)  # albedo_bins is not read without an albedo buffer
    p0 = np.zeros((height, width), dtype=RECORD)
    check(lib().pyr_render_features(world.scene(0), C.byref(cam.c), C.byref(desc), C.byref(fp0), None, p0.ctypes.data))
    assert p0.tobytes() == p1.tobytes()
    assert lib().pyr_render_features(world.scene(0), C.byref(cam.c), C.byref(desc), C.byref(fp), None, None) == abi.PYR_ERR_INVALID_ARGUMENT


def test_the_device_entry_writes_the_host_entry_bytes(gpu_lib):
    import torch

    world, cam, r, (width, height), _ = case("c3_shaped")
    a, p = raw_features(world, cam, (width, height), 3, 16)
    desc, fp = abi.PyrFilmDesc(width, height, 64, 380.0, 400.0), abi.PyrFeatureParams(3, 16)
    albedo = torch.zeros(height, width, 16, 2, dtype=torch.float32, device="cuda")
    records = torch.zeros(height, width, 8, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream()
    check(lib().pyr_render_features_device(world.scene(0), C.byref(cam.c), C.byref(desc), C.byref(fp), C.c_void_p(albedo.data_ptr()), C.c_void_p(records.data_ptr()),
                                           C.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    assert albedo.cpu().numpy().tobytes() == a.tobytes()
    assert records.cpu().numpy().tobytes() == p.tobytes()


def test_a_session_gives_the_same_features_and_keeps_its_film(gpu_lib):
    world, cam, r, (width, height) = c2_case()  # a world of its own: a session takes the scene
    r.pixel_samples = 8
    plain = r.features((width, height), cam, world, grid=3, albedo_bins=5)
    one_shot = r.new_film(width, height)
    r.render(one_shot, cam, world)
    with r.session((width, height), cam, world) as s:
        before = s.features(grid=3, albedo_bins=5)
        s.render(4)
        between = s.features(grid=3, albedo_bins=5)
        s.render(4)
        s.sync()
        film = s.film()
    for got in (before, between):
        assert got.records.tobytes() == plain.records.tobytes() and got.albedo.grains.tobytes() == plain.albedo.grains.tobytes()
    assert_same_film(film, one_shot, "session with two feature passes against one shot")
    world.close()


def test_the_render_is_untouched_by_a_feature_pass(gpu_lib):
    world, cam, r, (width, height) = c2_case()
    r.features((width, height), cam, world, grid=3, albedo_bins=16)
    film, cpu = r.new_film(width, height), r.new_film(width, height)
    r.render(film, cam, world)
    oracle.OracleScene(world).render(r, cam, cpu, threads=8)
    assert_same_film(film, cpu, "C2 render after a feature pass against the oracle")
    world.close()


def read_png(path):
    """uint8 [h, w, 3] of an 8-bit RGB PNG whose rows use filter 0 (what both front ends write)."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, idat, size = 8, b"", None
    while at < len(data):
        n, tag = int.from_bytes(data[at:at + 4], "big"), data[at + 4:at + 8]
        body = data[at + 8:at + 8 + n]
        if tag == b"IHDR":
            size = (int.from_bytes(body[:4], "big"), int.from_bytes(body[4:8], "big"))
            assert body[8:10] == b"\x08\x02"
        if tag == b"IDAT":
            idat += body
        at += 12 + n
    w, h = size
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape(h, w, 3)


def test_both_command_lines_write_the_feature_images(tmp_path, gpu_lib):
    project_file = os.path.join(PROJECTS, "gallery.lua")
    py_prefix, cpp_prefix = str(tmp_path / "py"), str(tmp_path / "cpp")
    py = subprocess.run([sys.executable, "-m", "pyrite_amd", project_file, "--size", "48x32", "--spp", "1", "--seed", "1", "-o", str(tmp_path / "py.png"), "--features", py_prefix],
                        cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
    assert py.returncode == 0, py.stderr
    cpp = subprocess.run([gpu_build.HOST_TOOL, "render-project", project_file, "-", "1", str(tmp_path / "cpp.png"), "--size", "48x32", "--spp", "1", "--features", cpp_prefix,
                          "--features-grid", "1"], cwd=ROOT, capture_output=True, text=True)
    assert cpp.returncode == 0, cpp.stderr
    project, base_dir = lua_project.load_project(project_file)
    project.setdefault("image", {}).update(width=48, height=32)
    world, cam, r, film = scenes.build(project, seed=1, base_dir=base_dir)
    got = r.features((48, 32), cam, world)
    image = project.get("image") or {}
    want = {"albedo": develop(got.albedo, filter=image.get("filter"), white=image.get("white")), "normal": encode_normal(got.normal, got.coverage),
            "depth": encode_depth(got.depth, got.coverage)}
    for kind, pixels in want.items():
        from_py, from_cpp = read_png(py_prefix + "_%s.png" % kind), read_png(cpp_prefix + "_%s.png" % kind)
        assert np.array_equal(from_py, pixels), kind
        assert np.array_equal(from_cpp, from_py), kind
    assert want["normal"].any() and want["depth"].any() and want["albedo"].any()
    world.close()
