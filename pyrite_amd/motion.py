"""Motion records (include/pyrite_gpu.h "motion records and accumulation over frames"): what
Renderer.motion and Session.motion return -- per pixel, where the surface point the camera sees was in the previous frame -- and
the host helper that inverts a camera. develop.reproject accumulates linear images along these records."""
import ctypes as C

import numpy as np

from . import abi
from ._lib import check, lib

RECORD = np.dtype([("prev_x", "<f4"), ("prev_y", "<f4"), ("prev_depth", "<f4"), ("depth", "<f4"), ("shape", "<u4"), ("flags", "<u4"), ("reserved", "<u4", (2,))])
assert RECORD.itemsize == 32 == C.sizeof(abi.PyrMotionPixel)
HIT, IN_FRONT, INSIDE = abi.PYR_MOTION_HIT, abi.PYR_MOTION_IN_FRONT, abi.PYR_MOTION_INSIDE


def world_to_cam(camera):
    """float32 [16], column-major: pyr_camera_world_to_cam of a renderer.Camera or an abi.PyrCamera -- the very matrix the motion
    pass projects with. No GPU is touched."""
    c = getattr(camera, "c", camera)
    out = (C.c_float * 16)()
    check(lib().pyr_camera_world_to_cam(C.byref(c), out))
    return np.array(out[:], dtype=np.float32)
