"""A guard on the code the compiler makes of the BASELINE kernel, run on the CPU (hipcc cross-compiles): render_kernel_sm for the
big non-interpreter scenes sits at 128 VGPRs with ~100 uniform words live across its stage loop against 104 SGPRs, and what does
not fit is parked in VGPR lanes and fetched back with v_readlane -- vector instructions in the hot phases. Round 4 saw ONE more
uniform bool kept across the loop turn 140 v_readlane into 387 and C3 from 584 into 559 Msamples/s while every test stayed
green; this test would have said so without a GPU. The synchronous walk of C1 / C2 tells the same story: stating its scattering
rule through the path's shared rules (kernels.hip) turns its 139 v_readlane into 206 for the same arithmetic."""
import os
import re
import subprocess

import pytest

from pyrite_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    out = tmp_path_factory.mktemp("isa") / "main.s"
    subprocess.check_call([build.HIPCC] + flags + ["--cuda-device-only", "-S", "kernels/main.hip", "-o", str(out)], cwd=build.CSRC,
                          stderr=subprocess.DEVNULL)
    return out.read_text()


def kernel_figures(text, mangled, shown):
    """(vector instructions, v_readlane, VGPRs, scratch bytes) of the kernel whose mangled name starts with `mangled`."""
    start = re.search(r"^%s\w*:" % mangled, text, re.M)
    assert start, "%s is not in the listing" % shown
    body = text[start.start():]
    body = body[:body.index("s_endpgm")]
    lines = [l.strip() for l in body.splitlines()]
    valu = sum(1 for l in lines if l.startswith("v_"))
    readlane = sum(1 for l in lines if l.startswith("v_readlane"))
    meta = text[text.index(".amdhsa_kernel", text.index(mangled[1:])):]
    vgprs = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1))
    scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1))
    return valu, readlane, vgprs, scratch


@pytest.mark.timeout(600)
def test_the_baseline_kernel_keeps_its_registers(listing):
    valu, readlane, vgprs, scratch = kernel_figures(listing, "_ZN3pyr16render_kernel_smILb0ELb0ELb0ELb1E", "render_kernel_sm<false, false, false, true>")
    # round 4: 8,278 vector instructions, 140 v_readlane, 128 VGPRs, 272 B of scratch (the traversal stack's deep end: no spill)
    assert vgprs <= 128, vgprs
    assert scratch <= 272, scratch
    assert readlane <= 170, "SGPR spills grew: %d v_readlane (140 in round 4): a uniform value too many is live across the stage loop" % readlane
    assert valu <= 8500, valu


@pytest.mark.timeout(600)
def test_the_synchronous_walk_keeps_its_registers(listing):
    """render_kernel<false, true, false>: the kernel C1 and C2 run (kernels/main.hip pick_kernel)."""
    valu, readlane, vgprs, scratch = kernel_figures(listing, "_ZN3pyr13render_kernelILb0ELb1ELb0E", "render_kernel<false, true, false>")
    # before the path's rules were stated once (round 17's parent): 6,486 vector instructions, 139 v_readlane, 116 VGPRs, no scratch.
    # Registers and scratch are bounded there; the counts have the headroom the case above gives its own (170 / 140, 8,500 / 8,278).
    assert vgprs <= 116, vgprs
    assert scratch <= 0, scratch
    assert readlane <= 168, "SGPR spills grew: %d v_readlane (139 before): a uniform value too many is live across the bounce" % readlane
    assert valu <= 6659, valu
