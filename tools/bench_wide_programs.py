#!/usr/bin/env python3
"""Developer tool (GPU box): throughput of the wide interpreter build -- scenes.wide_program_project with nine textures (12 RGB registers
after allocation: the wide build) against five (8: the in-register build), on spheres and on the torus knot, 256 x 256 x 16 spp. A plain
normal map in both, so that only the colour programs differ.     python tools/bench_wide_programs.py"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyrite_amd import scenes  # noqa: E402

for mesh in (False, True):
    for n in (9, 5):
        project = scenes.wide_program_project(mesh, textures=n, width=256, height=256, pixel_samples=16, spectrum_samples=8, layered=False)
        world, cam, r, film = scenes.build(project, seed=1)
        info = r.program_info(world)
        r.render(film, cam, world)  # warm-up
        times = []
        for _ in range(5):
            f = r.new_film(256, 256)
            t0 = time.perf_counter()
            r.render(f, cam, world)
            times.append(time.perf_counter() - t0)
        best = min(times)
        print("mesh=%d textures=%d wide=%d allocated=(%d,%d,%d) best %.2f ms  %.1f Msamples/s" % (
            mesh, n, info["wide"], info["allocated_numbers"], info["allocated_vectors"], info["allocated_rgbs"], best * 1e3, 256 * 256 * 16 / best / 1e6))
