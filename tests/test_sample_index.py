"""csrc/sample_index.h, the render MLP's division-free sample -> ray index and its exact reciprocal
of a power-of-two scale, checked without a GPU: tests/sample_index_check.cpp is compiled with the host
C++ compiler and compares the helpers with `/`, `%` and the float division: every N in 1..4096, 2^30 and
2^31 - 1 at the dividends around the multiples of N and at 2^31 - 1; the samples of 10,000 block steps
of three grid sizes; every scale pow2_scale returns against 10^6 random constants and the seeded
model's packed layer constants, which the kernel divides by those scales."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import REPO

CSRC = os.path.join(REPO, "depth-aware-shader-effects-for-nerf_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    path = str(tmp_path_factory.mktemp("sample_index") / "sample_index_check")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I", CSRC,
                    os.path.join(REPO, "tests", "sample_index_check.cpp"), "-o", path], check=True)
    return path


def seeded_constants(exe):
    """The nine constants 2^(e_w - 14) of the seeded model, as the host packer stores them."""
    import nerfmi
    from test_capi_host import host_pack
    torch.manual_seed(0)
    model = nerfmi.NeRF(nerfmi.Config()).eval()
    packed = host_pack({k: v.detach() for k, v in model.state_dict().items()})
    off, n = map(int, subprocess.run([exe, "--layout"], check=True, capture_output=True, text=True).stdout.split()[1:])
    cst = packed[off:off + n]
    assert (cst > 0).all() and (np.frexp(cst)[0] == 0.5).all(), cst   # powers of two, all set
    return cst


def test_helpers_match_the_operators(exe):
    cst = seeded_constants(exe)
    out = subprocess.run([exe] + [f"{int(b):08x}" for b in cst.view(np.uint32)], capture_output=True, text=True)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and not any(ln.startswith("FAIL") for ln in lines), out.stdout
    got = {ln.split()[1]: ln.split()[2:] for ln in lines if ln.startswith("ok")}
    assert set(got) == {"div_points", "div_steps", "recip"}
    assert int(got["div_points"][0]) > 4098 * 60            # every N, its dividends
    assert int(got["div_steps"][0]) == 3 * 7 * 10000 * 8    # 10,000 steps of three grids
    # 201 scales x (the given constants + 10^6 random ones), and the model's nine were among them
    assert int(got["recip"][0]) >= 201 * (1000000 + len(cst)) and int(got["recip"][2]) == len(cst) == 9
