"""k_copy's resident window without a GPU: the rule and the knob as a
stand-alone host program under the host sanitizers, and the emitted code of
k_copy_win and k_copy (a device-only cross-compile to assembly).
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM", "/opt/rocm")
HIPCC = shutil.which("hipcc") or os.path.join(ROCM, "bin", "hipcc")


def test_window_rule_and_knob_under_the_host_sanitizers(tmp_path):
    """tools/copy_window_host_check.cpp: around every threshold of
    copy_window_rule the window is at most the period, unit and period are
    powers of two, the resident bytes stay under the cap, the window never
    grows with n and is on over one range of sizes; copy_window_parse takes
    the documented forms and refuses the rest.  Built with
    -fsanitize=address,undefined and run once (nothing is loaded into python)."""
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "copy_window_host_check"
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include",
                    "-I" + os.path.join(ROOT, "mpi-perf_amd", "csrc"),
                    os.path.join(ROOT, "tools", "copy_window_host_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True, timeout=300)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-1500:])
    assert "copy_window_host_check: ok" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def test_k_copy_win_keeps_both_load_policies_and_nontemporal_stores(tmp_path):
    """Two loads of one pointer that differ only in the nontemporal hint are
    merged into one plain load, which silently makes the whole copy the
    default-policy form.  In the body of k_copy_win alone: at least one 16-byte
    load with nt and at least one without, and every 16-byte store with nt.
    In the body of k_copy, the form without the choice: every 16-byte load and
    store with nt."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    asm = tmp_path / "mpx_kernels.s"
    csrc = os.path.join(ROOT, "mpi-perf_amd", "csrc")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", f"-I{csrc}",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(csrc, "mpx_kernels.hip"), "-o", str(asm)],
                   check=True, capture_output=True, text=True, timeout=600)
    bodies, name = {}, None
    for line in asm.read_text().splitlines():
        m = re.match(r"^(_ZN3mpx(?:10k_copy_win|6k_copyI)\w+):", line)
        if m:
            name = m.group(1)
            bodies[name] = []
        elif name and re.match(r"^\s+s_endpgm\b", line):
            name = None
        elif name:
            bodies[name].append(line.split(";")[0].strip())
    win = [b for n, b in bodies.items() if "10k_copy_win" in n]
    plain = [b for n, b in bodies.items() if "6k_copyI" in n]
    assert len(win) == 1 and len(plain) == 1, sorted(bodies)

    def ops(body, kind):
        return [ln for ln in body if re.match(rf"(global|buffer|flat)_{kind}_dwordx4\b", ln)]

    def nt(ln):
        return re.search(r"\bnt\b", ln) is not None

    loads, stores = ops(win[0], "load"), ops(win[0], "store")
    assert any(nt(ln) for ln in loads), loads
    assert any(not nt(ln) for ln in loads), loads
    assert stores and all(nt(ln) for ln in stores), stores
    loads, stores = ops(plain[0], "load"), ops(plain[0], "store")
    assert loads and all(nt(ln) for ln in loads), loads
    assert stores and all(nt(ln) for ln in stores), stores
