"""The whole-database scan builds its argmin keys (distance << 7 | index, < 2^16) with v_fmaak_f32 on f32 bit patterns
that are denormals, and is exact only while the code object keeps f32 denormals.  A flag that flushes them would turn
every key into 0 and the match counts silently wrong, so compile the scan sources with the library's own flags and check
the float mode of every k_db_scan* kernel (CPU only: hipcc cross-compiles for gfx950)."""
import importlib.util
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nclt-slam-project_amd")


def _build_module():
    spec = importlib.util.spec_from_file_location("reloc_build_flags", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_scan_kernels_keep_f32_denormals(tmp_path):
    b = _build_module()
    text = ""
    for stem in ("reloc_scan", "reloc_scan_rows"):          # the count / emit family and the lane-per-row kernel
        asm = tmp_path / (stem + ".s")
        src = os.path.join(b.CSRC, stem + ".hip")
        r = subprocess.run([b.HIPCC] + b.FLAGS + ["-S", "--cuda-device-only", "-o", str(asm), src], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        text += asm.read_text()
    # one .amdhsa_kernel block per kernel: name, then its descriptor fields up to .end_amdhsa_kernel
    blocks = re.findall(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, flags=re.M | re.S)
    scan = [(name, body) for name, body in blocks if re.match(r"_Z\d+k_db_scan", name)]
    assert len(scan) >= 14, [name for name, _ in blocks]
    # by name: the count kernels, the six emit instantiations (NJ x waves), both batch kernels and the three lane-per-row ones
    want = [f"_Z9k_db_scanILi{nj}EEv" for nj in (2, 4, 8)]
    want += [f"_Z14k_db_scan_emitILi{nj}ELi{nw}EEv" for nj in (2, 4, 8) for nw in (4, 8)]
    want += ["_Z15k_db_scan_batch", "_Z20k_db_scan_emit_batch"]
    want += [f"_Z14k_db_scan_rowsILi{g}ELb{h}EEv" for g, h in ((4, 1), (8, 0), (16, 0))]
    missing = [w for w in want if not any(name.startswith(w) for name, _ in scan)]
    assert not missing, (missing, [name for name, _ in scan])
    for name, body in scan:
        m = re.search(r"\.amdhsa_float_denorm_mode_32\s+(\d+)", body)
        assert m and m.group(1) == "3", f"{name}: f32 denormals not preserved ({m.group(0) if m else 'no mode field'})"
    # and the keys are the FMA form this guard is about
    assert "v_fmaak_f32" in text
