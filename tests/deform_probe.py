"""The host rehearsal of a live scene's deformation pipeline (tests/probes/deform_check.cpp), for the four tests/test_scene_*_cpu.py:
building the probe with the sanitizers, writing its input -- a stage a case does not use has a count of zero -- running it as a child
process and reading what it wrote."""
import os
import subprocess

import numpy as np

import morph_restatement
import pose_restatement
import skin_restatement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("positions", "normals", "frames", "spheres")


def build(directory):
    exe = os.path.join(str(directory), "deform_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "probes", "deform_check.cpp")])
    return exe


def write_input(path, rest, ranges, lamps, poses={}, skins={}, joints={}, morphs={}, weights={}, smoothing={}):
    nt, ns = len(rest["positions"]), len(rest["spheres"])
    with open(path, "wb") as f:
        f.write(np.array([nt, ns, 0 if rest["frames"] is None else 1, len(ranges), len(lamps), len(skins), len(morphs), len(smoothing)], dtype=np.uint32).tobytes())
        for key in KEYS:
            if rest[key] is not None:
                f.write(np.ascontiguousarray(rest[key], dtype=np.float32).tobytes())
        for k, r in enumerate(ranges):
            matrix, scale = poses.get(k, (None, 1.0))
            f.write(np.array([r["first_triangle"], r["num_triangles"], r["first_sphere"], r["num_spheres"]], dtype=np.uint32).tobytes())
            f.write(pose_restatement.column_major(matrix).tobytes())
            f.write(np.float32(scale).tobytes())
        f.write(np.array(lamps, dtype=np.uint32).reshape(-1, 2).tobytes())
        for index in sorted(skins):
            skin = skins[index]
            f.write(np.array([index, skin["num_joints"]], dtype=np.uint32).tobytes())
            f.write(skin_restatement.joint_table(joints.get(index), skin["num_joints"]).tobytes())
            f.write(np.ascontiguousarray(skin["weights"], dtype=np.float32).tobytes())
            f.write(np.ascontiguousarray(skin["joints"], dtype=np.uint16).tobytes())
        for index in sorted(morphs):
            morph = morphs[index]
            f.write(np.array([index, len(morph["positions"]), 0 if morph["normals"] is None else 1], dtype=np.uint32).tobytes())
            f.write(morph_restatement.weights_of(weights, index, len(morph["positions"])).tobytes())
            f.write(np.ascontiguousarray(morph["positions"], dtype=np.float32).tobytes())
            if morph["normals"] is not None:
                f.write(np.ascontiguousarray(morph["normals"], dtype=np.float32).tobytes())
        for index in sorted(smoothing):
            f.write(np.array([index], dtype=np.uint32).tobytes())
            f.write(np.ascontiguousarray(smoothing[index], dtype=np.uint32).tobytes())


def read_output(path, rest, num_lamps):
    data = np.fromfile(path, dtype=np.float32)
    out, at = {}, 0
    for key in KEYS:
        if rest[key] is None:
            out[key] = None
            continue
        out[key] = data[at:at + rest[key].size].reshape(rest[key].shape)
        at += rest[key].size
    out["lamps"] = data[at:at + 23 * num_lamps].reshape(num_lamps, 23)
    at += 23 * num_lamps
    assert at + 1 == len(data)
    out["flag"] = int(data[at:].view(np.uint32)[0])
    return out


def rehearse(exe, tmp_path, name, rest, ranges, lamps, **stages):
    source, result = str(tmp_path / (name + ".in")), str(tmp_path / (name + ".out"))
    write_input(source, rest, ranges, lamps, **stages)
    run = subprocess.run([exe, source, result], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    return read_output(result, rest, len(lamps))
