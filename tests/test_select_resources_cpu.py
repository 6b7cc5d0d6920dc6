"""CPU test (no GPU) of the selection kernels' resources, read from the kernel metadata of t1k_assign.hip compiled for gfx950 with the
Makefile's flags (as tests/test_kernel_resources_cpu.py does for the chain): k_select<CAP, NT, XL, PK, CUT>.
  * No instantiation loses occupancy against the table of the selection before the size classes
    (profiles/r08_kernel_resources_select_tail.txt: seven wavefronts per SIMD for the 256-thread shape, eight for the 1024-thread shape),
    by registers and by LDS (static + the dynamic key array, 160 KB a compute unit).
  * The packed form without the cut's code (PK, !CUT: the launch over the lists of at most 1000 candidates) has no more scratch than the
    unpacked 256-thread form of the same build (12 bytes each; the parent's packed form had 108)."""
import re
import shutil
import subprocess

import pytest

import test_kernel_resources_cpu as kr

LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def select_kernels(tmp_path_factory):
    hipcc, flags = kr.hipcc_and_flags()
    if shutil.which(hipcc) is None:
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("res") / "t1k_assign.s")
    r = subprocess.run([hipcc] + flags + ["--offload-device-only", "-S", "-o", out, "t1k_assign.hip"], cwd=kr.CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    found = {}
    for name, k in kr.kernel_metadata(open(out).read()).items():
        # k_select<CAP, NT, XL, PK, CUT>(SelectArgs): _Z8k_selectILi<CAP>ELi<NT>ELb<XL>ELb<PK>ELb<CUT>EEv10SelectArgs
        m = re.match(r"_Z8k_selectILi(\d+)ELi(\d+)ELb([01])ELb([01])ELb([01])EEv", name)
        if m:
            found[tuple(int(x) for x in m.groups())] = k
    for key, k in sorted(found.items()):
        print("k_select<%d, %d, %d, %d, %d>: %s VGPRs, %s spilled, %s bytes of scratch, %s bytes of static LDS" % (key + (k[".vgpr_count"], k[".vgpr_spill_count"], k[".private_segment_fixed_size"], k[".group_segment_fixed_size"])))
    # per XL: the unpacked form of both shapes, the packed form without the cut, the packed form with the cut in both shapes
    assert sorted(found) == sorted((cap, nt, xl, pk, cut) for xl in (0, 1) for cap, nt, pk, cut in ((2048, 256, 0, 0), (8192, 1024, 0, 0), (2048, 256, 1, 0), (2048, 256, 1, 1), (8192, 1024, 1, 1)))
    return found


def occupancy(cap, nt, k):
    """wavefronts per SIMD that the registers and the LDS admit"""
    vgprs = (int(k[".vgpr_count"]) + 7) // 8 * 8
    by_regs = min(8, 512 // vgprs)
    by_lds = LDS_PER_CU // (int(k[".group_segment_fixed_size"]) + cap * 8) * (nt // 64) // 4
    return min(by_regs, by_lds)


def test_no_select_instantiation_loses_occupancy(select_kernels):
    for (cap, nt, xl, pk, cut), k in select_kernels.items():
        assert occupancy(cap, nt, k) >= (7 if nt == 256 else 8), ((cap, nt, xl, pk, cut), k)


def test_packed_form_without_the_cut_has_the_unpacked_forms_scratch(select_kernels):
    for xl in (0, 1):
        lean, unpacked = select_kernels[(2048, 256, xl, 1, 0)], select_kernels[(2048, 256, xl, 0, 0)]
        assert int(lean[".private_segment_fixed_size"]) <= int(unpacked[".private_segment_fixed_size"]), (xl, lean, unpacked)
