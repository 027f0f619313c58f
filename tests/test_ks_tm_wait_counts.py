"""k_mfma_ks_tm keeps k_mfma_ks's property (tests/test_ks_wait_counts.py): every iteration of a step
loop issues the same L = CT + 1 + 2 * MAXG loads per slot -- here CT = 2 16-byte units of X straight
into the MFMA's B registers, the step record and the groups -- so no `s_waitcnt vmcnt(n)` inside a
step loop has n < L * (D - 1), and nothing spills.  CPU test: reads the compiler's assembly for
gfx950, runs nothing."""
import os
import re
import subprocess

import pytest

from test_ks_wait_counts import CSRC, HIPCC, kernel_bodies, loads_per_slot, step_loops, vm_waits

TM_ARGS = ("const uint32_t *, const u32x4 *, const u32x4 *, const u32x2 *, const {et} *, {et} *, uint32_t, uint32_t, uint32_t, "
           "uint32_t, uint32_t, uint32_t, uint32_t, float *, uint32_t *, uint32_t, epilogue")
UNIT = f"""#include "hip_code/mfma_ks_tm.hpp"
namespace gsk {{
template __global__ void k_mfma_ks_tm<3, 8, 2, 1, 1, f16>({TM_ARGS.format(et="f16")});
template __global__ void k_mfma_ks_tm<7, 8, 2, 3, 0, bf16>({TM_ARGS.format(et="bf16")});
template __global__ void k_mfma_ks_tm<8, 8, 2, 4, 0, f16>({TM_ARGS.format(et="f16")});
}}
"""
# mangled-name prefix -> (MAXG, D)
KERNELS = {
    "_ZN3gsk12k_mfma_ks_tmILi3ELi8ELi2ELi1E": (1, 2),
    "_ZN3gsk12k_mfma_ks_tmILi7ELi8ELi2ELi3E": (3, 2),
    "_ZN3gsk12k_mfma_ks_tmILi8ELi8ELi2ELi4E": (4, 2),
}


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    d = tmp_path_factory.mktemp("ks_tm_waits")
    src, out = d / "ks_tm_waits.hip", d / "ks_tm_waits.s"
    src.write_text(UNIT)
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-result",
                           "-Wno-unused-command-line-argument", "-D__HIP_PLATFORM_AMD__", "-mllvm",
                           "-amdgpu-kernarg-preload-count=16", "-I", CSRC, "-S", "--cuda-device-only", str(src), "-o", str(out)])
    return out.read_text()


@pytest.mark.parametrize("prefix", sorted(KERNELS))
def test_step_loops_leave_the_other_slots_loads_in_flight(listing, prefix):
    MAXG, D = KERNELS[prefix]
    L = loads_per_slot(2, MAXG)
    bodies = [v for k, v in kernel_bodies(listing).items() if k.startswith(prefix)]
    assert len(bodies) == 1, f"{prefix}: {len(bodies)} kernels in the listing"
    lines = bodies[0]
    loops = step_loops(lines)
    # the fast loop and the general loop at least, each a whole round of D steps: D * L loads
    rounds = [(a, b) for a, b in loops if sum("global_load" in x for x in lines[a:b + 1]) >= D * L]
    assert len(rounds) >= 2, f"{prefix}: step loops not found ({loops})"
    seen = 0
    for a, b in loops:
        waits = vm_waits(lines[a:b + 1])
        print(f"{prefix} loop lines {a}..{b}: vmcnt waits {waits}")
        seen += len(waits)
        assert all(w >= L * (D - 1) for w in waits), (
            f"{prefix}: a step loop waits for vmcnt below L * (D - 1) = {L * (D - 1)}: {waits}")
    assert seen, f"{prefix}: no vmcnt waits in the step loops"
    # the B fragments come from global memory: no transposing LDS read, no B stage
    assert not any("ds_read_b64_tr" in x for x in lines), prefix


def test_no_scratch(listing):
    sizes = [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", listing)]
    spills = [int(x) for x in re.findall(r"\.vgpr_spill_count:\s*(\d+)", listing)]
    assert len(sizes) == len(KERNELS) and len(spills) == len(KERNELS), (sizes, spills)
    assert not any(sizes) and not any(spills), (sizes, spills)
