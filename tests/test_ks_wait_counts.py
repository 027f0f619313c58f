"""k_mfma_ks keeps its look-ahead loads in flight across the step loop (CPU test: reads the compiler's
assembly for gfx950, runs nothing).

ks_body keeps D register sets ("slots"); step i runs on slot i % D, which is then reloaded with step
i + D.  A slot issues L vector-memory loads: the step's B loads, 1 step record and 2 per group load
(positions, values).  In steady state the youngest load a step has to wait for has the L * (D - 1)
loads of the other slots behind it, so inside a step loop no `s_waitcnt vmcnt(n)` may have
n < L * (D - 1): a smaller one drains loads issued for later steps, and vmcnt(0) drains the whole
queue once per round (what the loops did while the prologue issued its loads in another order than
the loop body: the waits are the compiler's, merged over the loop's predecessors).

One small translation unit instantiates three kernels with the flags the engine's ks_launch object
gets:
- C2's k_mfma_ks<2,3,8,2,1,false,true,kKsPosU16,1,f16>: L = 2 + 1 + 2 = 5;
- the layer's k_mfma_ks_group<2,7,8,2,3,...>: L = 2 + 1 + 6 = 9;
- a 128-column kernel, k_mfma_ks<8,2,8,2,1,...>: L = 8 + 1 + 2 = 11.
A step loop is a backward branch whose body holds both MFMAs and global loads (the fast loop, the
general loop and whatever copies of them the compiler makes); every one of them is checked.
"""
import os
import re
import subprocess

import pytest

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "generalsparse_amd", "csrc")

KS_ARGS = ("const uint32_t *, const u32x4 *, const u32x4 *, const u32x2 *, const f16 *, f16 *, uint32_t, uint32_t, "
           "uint32_t, uint32_t, uint32_t, uint32_t, float *, uint32_t *, uint64_t *, uint32_t, const uint8_t *, epilogue")
UNIT = f"""#include "hip_code/mfma_ks.hpp"
namespace gsk {{
template __global__ void k_mfma_ks<2, 3, 8, 2, 1, false, true, kKsPosU16, 1, f16>({KS_ARGS});
template __global__ void k_mfma_ks_group<2, 7, 8, 2, 3, kKsPosU16, true, 0, f16>(ks_group_args);
template __global__ void k_mfma_ks<8, 2, 8, 2, 1, false, true, kKsPosU16, 0, f16>({KS_ARGS});
}}
"""
# mangled-name prefix -> (CT, MAXG, D)
KERNELS = {
    "_ZN3gsk9k_mfma_ksILi2ELi3ELi8ELi2ELi1E": (2, 1, 2),
    "_ZN3gsk15k_mfma_ks_groupILi2ELi7ELi8ELi2ELi3E": (2, 3, 2),
    "_ZN3gsk9k_mfma_ksILi8ELi2ELi8ELi2ELi1E": (8, 1, 2),
}


def loads_per_slot(CT, MAXG):
    return CT + 1 + 2 * MAXG


def kernel_bodies(text):
    """{mangled name: the lines from the kernel's label to its .end_amdhsa_kernel}"""
    out, cur = {}, None
    for ln in text.splitlines():
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None:
            if ".end_amdhsa_kernel" in ln:
                cur = None
            else:
                cur.append(ln)
    return out


def step_loops(lines):
    """[(first, last)] line ranges of the backward branches whose body has MFMAs and global loads"""
    label = {}
    for i, ln in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            label[m.group(1)] = i
    out = []
    for i, ln in enumerate(lines):
        m = re.search(r"\bs_c?branch\w*\s+(\.LBB\d+_\d+)", ln)
        if m and label.get(m.group(1), i) < i:
            body = lines[label[m.group(1)]:i + 1]
            if any("v_mfma" in x for x in body) and any("global_load" in x for x in body):
                out.append((label[m.group(1)], i))
    return out


def vm_waits(lines):
    return [int(m.group(1)) for m in (re.search(r"\bs_waitcnt\b.*\bvmcnt\((\d+)\)", x) for x in lines) if m]


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    d = tmp_path_factory.mktemp("ks_waits")
    src, out = d / "ks_waits.hip", d / "ks_waits.s"
    src.write_text(UNIT)
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-result",
                           "-Wno-unused-command-line-argument", "-D__HIP_PLATFORM_AMD__", "-mllvm",
                           "-amdgpu-kernarg-preload-count=16", "-I", CSRC, "-S", "--cuda-device-only", str(src), "-o", str(out)])
    return out.read_text()


@pytest.mark.parametrize("prefix", sorted(KERNELS))
def test_step_loops_leave_the_other_slots_loads_in_flight(listing, prefix):
    CT, MAXG, D = KERNELS[prefix]
    L = loads_per_slot(CT, MAXG)
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


def test_no_scratch(listing):
    """the three instantiations keep everything in registers"""
    sizes = [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", listing)]
    spills = [int(x) for x in re.findall(r"\.vgpr_spill_count:\s*(\d+)", listing)]
    assert len(sizes) == len(KERNELS) and len(spills) == len(KERNELS), (sizes, spills)
    assert not any(sizes) and not any(spills), (sizes, spills)
