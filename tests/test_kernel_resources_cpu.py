"""CPU test (no GPU): the closed-form pass of the chain, k_chain_fast<NW, 0>, must be compiled without register spills and without
scratch memory.  A build of it that was held to fewer registers (72 VGPRs, 32 of them spilled) was slower and gave wrong, varying results
(t1k_amd/csrc/t1k_dev.h, docs/HISTORY.md), and nothing else would notice a change of flags, compiler or code that brings the spills back:
the file is compiled for gfx950 with the Makefile's flags, device side only, and the resource figures are read from the kernel metadata of
the assembly.  The VGPR count itself is not pinned."""
import os
import re
import shutil
import subprocess

import pytest

import util

CSRC = os.path.join(util.ROOT, "t1k_amd", "csrc")


def makefile_var(name, text):
    return re.search(r"^%s \??= *(.*)$" % name, text, flags=re.M).group(1).strip()


def hipcc_and_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    hipcc = os.environ.get("HIPCC", makefile_var("HIPCC", text))
    flags = makefile_var("FLAGS", text).replace("$(EXTRA)", "").replace("$(ARCH)", makefile_var("ARCH", text))
    return hipcc, flags.split()


def kernel_metadata(asm):
    """{mangled kernel name: {key: value}} from the amdhsa.kernels list of a device assembly file"""
    meta = asm[asm.index(".amdgpu_metadata"):]
    kernels = {}
    for entry in re.split(r"\n  - (?=\.)", meta)[1:]:
        fields = dict(re.findall(r"^\s+(\.[a-z_]+):\s+(\S+)\s*$", "    " + entry, flags=re.M))
        if ".name" in fields and ".vgpr_count" in fields:
            kernels[fields[".name"]] = fields
    return kernels


def test_closed_form_kernel_keeps_its_registers(tmp_path):
    hipcc, flags = hipcc_and_flags()
    if shutil.which(hipcc) is None:
        pytest.skip("no hipcc")
    out = str(tmp_path / "t1k_chain.s")
    r = subprocess.run([hipcc] + flags + ["--offload-device-only", "-S", "-o", out, "t1k_chain.hip"], cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    kernels = kernel_metadata(open(out).read())
    for nw in (5, 10):
        # k_chain_fast<NW, 0>(ChainArgs, ...): Itanium name _Z12k_chain_fastILi<NW>ELi0E...
        mine = [k for k in kernels if re.match(r"_Z12k_chain_fastILi%dELi0E" % nw, k)]
        assert len(mine) == 1, (nw, sorted(kernels))
        k = kernels[mine[0]]
        print("k_chain_fast<%d, 0>: %s VGPRs, %s SGPRs, %s + %s spilled, %s bytes of scratch" % (nw, k[".vgpr_count"], k[".sgpr_count"], k[".vgpr_spill_count"], k[".sgpr_spill_count"], k[".private_segment_fixed_size"]))
        assert int(k[".private_segment_fixed_size"]) == 0, (mine[0], k)
        assert int(k[".vgpr_spill_count"]) == 0, (mine[0], k)
