"""Shapes and labels of the pyr_scene_set_smoothing tests (tests/test_scene_smooth_cpu.py on the host rehearsal,
tests/test_gpu_scene_smooth.py on the kernel): the shapes of tests/pose_cases.py, each smoothed object welded by the bits of its
rest positions and rest normals (tests/smooth_restatement.py weld).

  knot_one  the knot as ONE object, triangles(12, 640): 320 groups, all of valence 6 -- two workgroups, the second a partial one.
            Welded that way, its recomputed rest normals agree with its stored ones to within 1e-7 in cosine.
  knot      the knot in pose_cases' two-object split (288 and 352 triangles), both smoothed: 304 + 320 groups (the cut opens
            the seam), so the object boundary falls inside the second workgroup. Object 0 also carries the skin of
            tests/skin_cases.py, and both carry the morph of tests/morph_cases.py without normal deltas.
  cornell   74 groups of valence 1 and 2; 8 of its 36 triangles are wound against their normals and are negated.
  textures  2 triangles, 4 groups, frames under a normal map."""
import numpy as np

import morph_cases
import pose_cases as cases
import skin_cases
import smooth_restatement as restatement

f32 = np.float32

SHAPES = ("cornell", "textures", "knot", "knot_one")
GROUPS = {"cornell": [74], "textures": [4], "knot": [304, 320], "knot_one": [320]}
ONE_KNOT = [cases.triangles(12, cases.KNOT_TRIANGLES)]


def make(shape, seed=5):
    """(world, camera, renderer, film, ranges) of a shape, nothing smoothed yet."""
    if shape != "knot_one":
        return cases.build(shape, seed=seed)
    from pyrite_amd import scenes

    world, cam, r, film = scenes.build(cases.SHAPES["knot"][0](), seed=seed)
    world.set_objects(ONE_KNOT)
    return world, cam, r, film, world.objects


def smoothed_objects(shape, world):
    """The indices of the objects whose normals are recomputed."""
    return [0, 1] if shape == "knot" else [skin_cases.skinned_object(world)]


def labels_for(shape, world, rest, ranges):
    out = {}
    for index in smoothed_objects(shape, world):
        t0, n = ranges[index]["first_triangle"], ranges[index]["num_triangles"]
        out[index] = restatement.weld(rest["positions"][t0:t0 + n], rest["normals"][t0:t0 + n])
    return out


def build(shape, seed=5):
    """(world, camera, renderer, film, ranges, rest, smoothing) of a shape with its smoothing set; nothing touches a GPU before a
    scene is asked for."""
    world, cam, r, film, ranges = make(shape, seed=seed)
    rest = cases.rest_of(world)
    smoothing = labels_for(shape, world, rest, ranges)
    world.set_smoothing(smoothing)
    return world, cam, r, film, ranges, rest, smoothing


def morphs_for(shape, world, rest, ranges):
    """The targets of tests/morph_cases.py without normal deltas, for every smoothed object."""
    return {index: morph_cases.targets(rest, ranges[index], with_normals=False) for index in smoothed_objects(shape, world)}


def skins_for(shape, rest, ranges):
    return {0: skin_cases.bend(rest, ranges[0])} if shape in ("knot", "knot_one") else {}
