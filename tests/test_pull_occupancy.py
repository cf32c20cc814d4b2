"""CPU-only check of the register budget of the C1 step's two kernels (csrc/kge_pull.hip), read from the AMDGPU metadata of the
built library: k_pull_eval<L1, 32, 1> and k_pull_step<Adam, L1, 32, 1, DIR> must each fit 8 waves per SIMD (at most 64 VGPRs)
with no scratch and no spills.  At 8 waves per SIMD the evaluation's 2 048 workgroups are one residency round on the 256 CUs and
the owner launch holds 2 048 of its 2 173 workgroups at once (1 792 at 7 waves; DESIGN.md sections 3 and 9).

The code objects are taken out of the library's offload bundles and their metadata notes read with llvm-readelf from the ROCm
LLVM tools; the test skips where those are not installed."""
import os
import re
import shutil
import struct
import subprocess
import tempfile

import pytest

BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TARGET = "gfx950"
KERNELS = {
    "k_pull_eval<true, 32, 1>": "_ZN3kge11k_pull_evalILb1ELi32ELi1EEEv",
    "k_pull_step<Adam, true, 32, 1, true>": "_ZN3kge11k_pull_stepILi1ELb1ELi32ELi1ELb1EEEv",
}


def _readelf():
    p = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")
    return p if os.access(p, os.X_OK) else shutil.which("llvm-readelf")


def _code_objects(blob):
    """The gfx950 code objects of every (uncompressed) clang offload bundle in `blob`."""
    out = []
    pos = blob.find(BUNDLE_MAGIC)
    while pos >= 0:
        n, = struct.unpack_from("<Q", blob, pos + len(BUNDLE_MAGIC))
        q = pos + len(BUNDLE_MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, q)
            triple = blob[q + 24:q + 24 + tlen].decode("ascii", "replace")
            q += 24 + tlen
            co = blob[pos + off:pos + off + size]
            if triple.endswith("--" + TARGET) and co[:4] == b"\x7fELF":
                out.append(co)
        pos = blob.find(BUNDLE_MAGIC, pos + 1)
    return out


def _kernel_metadata(readelf, co):
    """{kernel name: {metadata key: value}} from the scalar entries of the code object's amdhsa.kernels notes."""
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(co)
        f.flush()
        notes = subprocess.run([readelf, "--notes", f.name], check=True, capture_output=True, text=True).stdout
    kernels, cur = {}, None
    for line in notes.splitlines():
        m = re.match(r"^  - \.(\w+):\s*(.*)$", line)    # first key of a kernel entry
        if m:
            cur = {m.group(1): m.group(2).strip()}
            continue
        m = re.match(r"^    \.(\w+):\s*(\S.*)$", line)   # the kernel's other scalar keys (its args sit deeper)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2).strip()
            if m.group(1) == "name":
                kernels[cur["name"]] = cur
    return kernels


@pytest.fixture(scope="module")
def metadata():
    readelf = _readelf()
    if readelf is None:
        pytest.skip("llvm-readelf (ROCm LLVM tools) not installed")
    from pykg2vec_amd import _lib
    with open(_lib.LIB_PATH, "rb") as f:
        blob = f.read()
    cos = _code_objects(blob)
    assert cos, "no %s code object found in %s" % (TARGET, _lib.LIB_PATH)
    md = {}
    for co in cos:
        md.update(_kernel_metadata(readelf, co))
    return md


@pytest.mark.parametrize("label", sorted(KERNELS))
def test_c1_kernel_fits_eight_waves_without_scratch(metadata, label):
    prefix = KERNELS[label]
    found = [k for k in metadata if k.startswith(prefix)]
    assert len(found) == 1, (label, found)
    md = metadata[found[0]]
    # (gfx90a and later: .vgpr_count is the unified total -- architectural VGPRs plus AGPRs -- that sets the occupancy)
    vgpr = int(md["vgpr_count"])
    assert vgpr <= 64, "%s: %d VGPRs (arch + acc): fewer than 8 waves per SIMD" % (label, vgpr)
    assert int(md["private_segment_fixed_size"]) == 0, "%s: %s bytes of scratch per lane" % (label, md["private_segment_fixed_size"])
    assert int(md["vgpr_spill_count"]) == 0 and int(md["sgpr_spill_count"]) == 0, (label, md["vgpr_spill_count"], md["sgpr_spill_count"])
    assert md.get("uses_dynamic_stack", "false") == "false", label
