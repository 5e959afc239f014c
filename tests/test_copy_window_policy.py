"""k_copy_win's cache policies in its emitted gfx950 code (no GPU: a
device-only cross-compile to assembly).

The source asks for three policies (mpx_kernels.hip): kept blocks load through
a buffer descriptor with aux kCopyWinKeptAux, streamed blocks with a
nontemporal pointer load, and every 16-byte store is a buffer store with aux
kCopyWinStoreAux.  Two accesses of one address that differ only in a hint can
be merged into one, which drops the hint without changing a byte; so the
modifiers are read where they end up.  Only their presence is checked.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM", "/opt/rocm")
HIPCC = shutil.which("hipcc") or os.path.join(ROCM, "bin", "hipcc")
CSRC = os.path.join(ROOT, "mpi-perf_amd", "csrc")
AUX_BITS = {1: "sc0", 2: "nt", 16: "sc1"}        # gfx940-family buffer cache policy bits
POLICY = {"sc0", "sc1", "nt"}


def mods_of_aux(aux):
    assert aux & ~sum(AUX_BITS) == 0, aux
    return frozenset(name for bit, name in AUX_BITS.items() if aux & bit)


def source_constant(name):
    text = open(os.path.join(CSRC, "mpx_kernels.hip")).read()
    m = re.search(rf"constexpr int {name} = (\d+);", text)
    assert m, name
    return int(m.group(1))


def test_aux_bits_map_to_the_modifiers_the_assembler_prints():
    assert mods_of_aux(0) == frozenset()
    assert mods_of_aux(18) == {"sc1", "nt"} and mods_of_aux(19) == {"sc0", "sc1", "nt"}


def test_k_copy_win_carries_each_policy_the_source_asks_for(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    asm = tmp_path / "mpx_kernels.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", f"-I{CSRC}",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(CSRC, "mpx_kernels.hip"), "-o", str(asm)],
                   check=True, capture_output=True, text=True, timeout=600)
    body, inside = [], False
    for line in asm.read_text().splitlines():
        if re.match(r"^_ZN3mpx10k_copy_win\w+:", line):
            inside = True
        elif inside and re.match(r"^\s+s_endpgm\b", line):
            break
        elif inside:
            body.append(line.split(";")[0].strip())
    assert body, "k_copy_win not found"

    def ops(kind):
        """(address space, policy modifiers) of every 16-byte access of that kind"""
        out = []
        for ln in body:
            m = re.match(rf"(global|buffer|flat)_{kind}_dwordx4\b(.*)", ln)
            if m:
                out.append((m.group(1), frozenset(re.findall(r"\b(sc0|sc1|nt)\b", m.group(2)))))
        return out

    kept = ("buffer", mods_of_aux(source_constant("kCopyWinKeptAux")))
    streamed = ("global", frozenset({"nt"}))
    store = ("buffer", mods_of_aux(source_constant("kCopyWinStoreAux")))
    loads, stores = ops("load"), ops("store")
    assert kept != streamed
    assert set(loads) == {kept, streamed}, loads      # both survive, neither merged into the other
    assert stores and set(stores) == {store}, stores
