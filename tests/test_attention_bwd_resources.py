"""Compile-time resource guard for the training attention kernels
(native/kernels/attention_train.hip; hipcc cross-compiles gfx950 on the CPU):
no spills, no scratch, and the occupancy each kernel's __launch_bounds__
declares. Same remark parsing as tests/test_kernel_resources.py."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HIPCC = "/opt/rocm/bin/hipcc"
SRC = ROOT / "native" / "kernels" / "attention_train.hip"

pytestmark = [pytest.mark.skipif(not Path(HIPCC).exists() and shutil.which("hipcc") is None,
                                 reason="hipcc not available"),
              pytest.mark.timeout(900)]

# kernel -> (workgroups per CU, waves per SIMD) its __launch_bounds__ declare
# (256 threads = 4 waves, one per SIMD, per workgroup)
DESIGN = {"fwd_lse": (2, 2), "bwd_dkdv": (1, 1), "bwd_dq": (2, 2)}


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    odir = tmp_path_factory.mktemp("attention_train")
    cmd = [HIPCC if Path(HIPCC).exists() else "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c",
           "-I", str(SRC.parent), str(SRC), "-o", str(odir / "attention_train.o"),
           "-Rpass-analysis=kernel-resource-usage", "-save-temps=obj"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=800, cwd=odir)
    assert out.returncode == 0, out.stderr[-2000:]
    (s_file,) = list(odir.glob("attention_train-hip-amdgcn-amd-amdhsa-gfx950.s"))
    res, name = {"asm": s_file.read_text()}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res.setdefault(name, {})
            continue
        m = re.search(r"\s([A-Za-z ]+?)(?: \[bytes/\w+\])?: (\d+) \[-Rpass", line)
        if m and name:
            res[name][m.group(1).strip()] = int(m.group(2))
    return res


def _kernel(res, short):
    (hit,) = [r for n, r in res.items() if re.search(rf"attn_train\d+{short}E", n)]
    return hit


def _body(res, short):
    asm = res["asm"]
    m = re.search(rf"\n(_ZN3kgs10attn_train\d+{short}E\S+):", asm)
    return asm[m.end():asm.find(".Lfunc_end", m.end())]


def _vregs(text: str) -> set:
    out = set()
    for a, b in re.findall(r"(?<![\w.])v\[(\d+):(\d+)\]", text):
        out |= set(range(int(a), int(b) + 1))
    out |= {int(a) for a in re.findall(r"(?<![\w.\[])v(\d+)\b", text)}
    return out


def _tr_read_hazards(body: str) -> list:
    """Instructions that name a VGPR a ``ds_read_b64_tr_b16`` is still filling,
    i.e. before the next ``s_waitcnt`` with ``lgkmcnt(0)`` (textual order) -- the
    check tests/test_kernel_resources.py applies to the transposed-layout GEMMs."""
    pending, bad = set(), []
    for ln in body.splitlines():
        code = ln.split(";")[0].strip()
        if not code or code.startswith(".") or code.endswith(":"):
            continue
        if code.startswith("s_waitcnt") and "lgkmcnt(0)" in code:
            pending = set()
        elif code.startswith("ds_read_b64_tr_b16"):
            dst, addr = code.split(None, 1)[1].split(",", 1)
            if _vregs(addr) & pending:
                bad.append(code)
            pending |= _vregs(dst)
        elif _vregs(code) & pending:
            bad.append(code)
    return bad


def test_the_four_kernels_are_there_and_no_second_production_forward(resources):
    for short in ("fwd_lse", "bwd_prep", "bwd_dkdv", "bwd_dq"):
        _kernel(resources, short)
    # tests/test_kernel_resources.py finds the production forward by "attn3fwd"
    assert not [n for n in resources if "attn3fwd" in n]


@pytest.mark.parametrize("short", ["fwd_lse", "bwd_prep", "bwd_dkdv", "bwd_dq"])
def test_no_spills_and_no_scratch(resources, short):
    r = _kernel(resources, short)
    assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, r
    assert r.get("ScratchSize", 0) == 0, r


def test_fwd_lse_meets_the_forwards_limits(resources):
    r = _kernel(resources, "fwd_lse")
    assert r["VGPRs"] + r.get("AGPRs", 0) <= 256  # 2 waves / SIMD
    assert r["LDS Size"] <= 80 * 1024            # 2 workgroups / CU (160 KiB)


@pytest.mark.parametrize("short", ["bwd_dkdv", "bwd_dq"])
def test_backward_kernels_meet_their_declared_occupancy(resources, short):
    wgs, waves = DESIGN[short]
    r = _kernel(resources, short)
    assert r["LDS Size"] <= 160 * 1024 // wgs, r
    assert r["VGPRs"] + r.get("AGPRs", 0) <= 512 // waves, r


def test_declared_occupancy_is_what_the_source_says():
    src = SRC.read_text()
    for short, (wgs, _) in DESIGN.items():
        assert re.search(rf"__launch_bounds__\(256, {wgs}\)[^\n]*void {short}\(", src), short


def test_dkdv_asm_tr_reads_are_waited_before_use_and_its_loop_keeps_the_dma_in_flight(resources):
    """bwd_dkdv runs one wave per SIMD, so it issues its transposed reads as
    inline asm (hipcc would drain the LDS-DMA before a builtin one) and waits
    for them itself: no instruction may touch a destination register before the
    lgkmcnt(0), and the only vector-memory waits left are the prologue's and
    the one that ends each tile (x 2: hipcc peels the first iteration)."""
    body = _body(resources, "bwd_dkdv")
    assert body.count("ds_read_b64_tr_b16") == 64
    assert _tr_read_hazards(body) == []
    code = [ln.split(";")[0].strip() for ln in body.splitlines()]
    waits = [ln for ln in code if ln.startswith("s_waitcnt") and "vmcnt" in ln]
    assert len(waits) <= 3 and all("vmcnt(0)" in ln for ln in waits), waits


def test_tr_read_hazard_check_catches_an_early_use():
    body = ("\tds_read_b64_tr_b16 v[10:11], v5\n\tv_mov_b32 v21, v11\n\ts_waitcnt lgkmcnt(0)\n")
    assert _tr_read_hazards(body) == ["v_mov_b32 v21, v11"]
