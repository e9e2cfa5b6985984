"""Shifted-window attention kernels (csrc/attention.hip, attention_mfma.hip, attention_common.h) against the float64 CPU
reference of tests/attention_ref.py, through hip.window_attention_fwd / _bwd, on padded NON-CUBIC grids: S != H != W, a
different padding per axis combined with a shift, head dims 8 / 16 / 32, every MFMA key-tile tier (NKT 1, 2, 4, 7, 11), the
MFMA forward feeding the vector backward (head dim 32 at window 7), a clamped window under a larger bias table, per-sample
tables.  B = 2 everywhere, the two samples differ, qkv_bias is non-zero.  DESIGN.md, "Window attention tests".

(a) `test_window_attention_routing_exact`: q = k = 0 and a bias table that is zero except ONE +300 spike per head, so the
scores depend on the addressing alone: a query whose spiked key lies inside its window beats every other key by >= 200 (even
across the -100 mask), exp(-200) is 0 in fp32, the probability row is exactly one-hot (also after bf16 rounding and after the
online-softmax rescaling), and the output EQUALS one V row: multiples of 1/8 in [-8, 8], exact in bf16.  An H / W swap, a
z / y / x swap in the bias code, a wrong head column, an off-by-one region boundary or a padded key read from memory fails an
equality, whatever the gates are.
(b) `test_window_attention_random_vs_float64`: randn operands rounded through the compute dtype; out, lse, dqkv, dtable under
two metrics: max |err| / max |ref|, and the WORST WINDOW (relative L2 per window, maximum over the windows; dtable: per head
column), which stops one bad window from being averaged away.
tests/test_attention_ref_host.py shows on the CPU that wrong variants of the reference are caught by (a) or by the gates of (b).

Every case prints the path it took.  The backward's path is asserted from the library's own rule
(msseg_window_attention_bwd_workspace_bytes > 0 <=> MFMA backward); the attention launches write no per-launch timer records, so
the forward's path and the tile tier are asserted from the dispatch rule of msseg_window_attention_fwd restated in `route`.
A case that cannot reach the path its row names fails."""
import functools
import os

import pytest
import torch

from tests.attention_ref import window_attention_ref
from tests.test_gpu_kernels import rnd

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DEV = "cuda:0"

# case: grid (S, H, W), window, shift, heads, head dim, window edge the bias table is built for
CASES = {
    "A": ((5, 8, 7), 3, 1, 3, 8, 3),       # head dim 8 never takes MFMA
    "B": ((9, 7, 13), 6, 3, 3, 16, 6),     # NKT 7 forward and backward
    "C": ((8, 15, 10), 7, 3, 2, 32, 7),    # NKT 11 forward feeding the VECTOR backward (the backward's LDS image does not fit)
    "D": ((6, 4, 9), 4, 2, 4, 16, 7),      # NKT 2, clamped-window index (bias_ws > ws)
    "E": ((7, 11, 5), 5, 2, 3, 16, 5),     # NKT 4, 125 tokens: a partly filled last tile
    "F": ((4, 6, 5), 3, 0, 2, 16, 3),      # NKT 1; padding without a mask
    "G": ((12, 6, 6), 6, 0, 2, 32, 6),     # MFMA backward at head dim 32; no padding
    "H": ((7, 14, 9), 7, 3, 3, 16, 7),     # NKT 11 forward and backward
}
# path: (dtype, environment switches)
PATHS = {
    "fp32": (F32, {}),
    "bf16": (BF16, {}),
    "bf16_no_ws": (BF16, {"MSSEG_ATTN_BWD_NO_WS": "1"}),
    "bf16_no_mfma": (BF16, {"MSSEG_ATTN_NO_MFMA": "1"}),
}
# (case, path) -> (forward kernel, backward kernel, MFMA tile tier or None) the row of the table must reach
EXPECT = {
    ("A", "fp32"): ("fp32_vector", "fp32_vector", None),
    ("A", "bf16"): ("bf16_vector", "bf16_vector", None),
    ("B", "fp32"): ("fp32_vector", "fp32_vector", None),
    ("B", "bf16"): ("bf16_mfma", "bf16_mfma_ws", 7),
    ("B", "bf16_no_ws"): ("bf16_mfma", "bf16_mfma_atomics", 7),
    ("B", "bf16_no_mfma"): ("bf16_vector", "bf16_vector", None),
    ("C", "bf16"): ("bf16_mfma", "bf16_vector", 11),
    ("C", "fp32"): ("fp32_vector", "fp32_vector", None),
    ("D", "bf16"): ("bf16_mfma", "bf16_mfma_ws", 2),
    ("E", "bf16"): ("bf16_mfma", "bf16_mfma_ws", 4),
    ("F", "bf16"): ("bf16_mfma", "bf16_mfma_ws", 1),
    ("G", "bf16"): ("bf16_mfma", "bf16_mfma_ws", 7),
    ("H", "bf16"): ("bf16_mfma", "bf16_mfma_ws", 11),
}
PER_SAMPLE_CASES = ("A", "B", "H")
RANDOM_RUNS = [(c, p, False) for c, p in EXPECT] + [(c, p, True) for c, p in EXPECT if c in PER_SAMPLE_CASES]
FWD_RUNS = [(c, p) for c, p in EXPECT if p != "bf16_no_ws"]          # the switch of that path acts on the backward only
# one case per backward form is also called with dtable = None and with dtable pre-filled with 0.5
CALL_FORMS = {("A", "fp32", False), ("B", "bf16", False), ("B", "bf16_no_ws", False)}

# Gates of (b): (max |err| / max |ref|, worst window) per kernel and tensor = 4 x the largest value measured on an MI355X against
# the float64 reference over every run of that kernel in this file, (a) included for `out` (the margin of SUMSQ_GATES in
# tests/test_gpu_conv_exact.py: run-to-run atomics order, other seeds).  No first number is looser than what the suite already
# uses for the same quantity: 2e-4 (fp32) / 3e-2 (bf16) for out and dqkv, 1e-3 / 5e-2 for dtable.
ATTN_GATES = {
    "fp32_vector": {
        "out": (3.1e-06, 1.3e-06),          # measured 7.713e-07, 3.129e-07
        "lse": (8.8e-07, 2.9e-07),          # measured 2.199e-07, 7.213e-08
        "dqkv": (1.7e-06, 1.9e-06),         # measured 4.242e-07, 4.678e-07
        "dtable": (1.3e-06, 1.7e-06),       # measured 3.164e-07, 4.204e-07
    },
    "bf16_vector": {
        "out": (1.5e-02, 8.2e-03),          # measured 3.576e-03, 2.035e-03
        "lse": (8.8e-07, 3.0e-07),          # measured 2.192e-07, 7.270e-08
        "dqkv": (9.2e-03, 8.3e-03),         # measured 2.277e-03, 2.065e-03
        "dtable": (5.3e-03, 5.8e-03),       # measured 1.319e-03, 1.443e-03
    },
    "bf16_mfma": {
        "out": (1.7e-02, 9.8e-03),          # measured 4.081e-03, 2.443e-03
        "lse": (7.6e-07, 3.0e-07),          # measured 1.882e-07, 7.443e-08
    },
    "bf16_mfma_ws": {
        "dqkv": (1.6e-02, 1.2e-02),         # measured 3.892e-03, 2.787e-03
        "dtable": (8.4e-03, 7.7e-03),       # measured 2.088e-03, 1.906e-03
    },
    "bf16_mfma_atomics": {
        "dqkv": (1.6e-02, 1.1e-02),         # measured 3.892e-03, 2.567e-03
        "dtable": (2.1e-03, 2.7e-03),       # measured 5.218e-04, 6.632e-04
    },
}
SUITE_CAPS = {F32: {"out": 2e-4, "dqkv": 2e-4, "dtable": 1e-3}, BF16: {"out": 3e-2, "dqkv": 3e-2, "dtable": 5e-2}}

SPIKE_OFFSETS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1)]
SPIKE = 300.0


# ------------------------------------------------------------------------------------------------------------------
# inputs and references (CPU only; cached per case)
# ------------------------------------------------------------------------------------------------------------------
def _threads():
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def spike_table(heads, bws):
    """float64 [M3, heads]: zero except +300 at query - key = SPIKE_OFFSETS[h % 6] on the grid the index was built for"""
    m = 2 * bws - 1
    t = torch.zeros(m ** 3, heads, dtype=torch.float64)
    for h in range(heads):
        dz, dy, dx = SPIKE_OFFSETS[h % 6]
        t[((dz + bws - 1) * m + dy + bws - 1) * m + dx + bws - 1, h] = SPIKE
    return t


def routing_inputs(case):
    """(qkv, qkv_bias, table) float64: zero q and k thirds (of the bias too), v thirds multiples of 1/8 in [-8, 8]"""
    (S, H, W), ws, shift, heads, hd, bws = CASES[case]
    C = heads * hd
    g = torch.Generator().manual_seed(100 + ord(case))
    qkv = torch.zeros(2, S, H, W, 3 * C, dtype=torch.float64)
    qkv[..., 2 * C:] = torch.randint(-64, 65, (2, S, H, W, C), generator=g).double() / 8
    qb = torch.zeros(3 * C, dtype=torch.float64)
    qb[2 * C:] = torch.randint(-64, 65, (C,), generator=g).double() / 8
    return qkv, qb, spike_table(heads, bws)


def routing_ref_of(inputs, case, _variant=None):
    (S, H, W), ws, shift, heads, hd, bws = CASES[case]
    qkv, qb, tab = inputs
    with torch.no_grad():
        out, lse, pmax = window_attention_ref(qkv, qb, tab, heads, ws, shift, bws, _variant=_variant)
    # float64 keeps exp(-200) ~ 1e-87 where fp32 has 0 (smallest subnormal 1.4e-45): on a one-hot row whose V value is 0 the
    # reference holds such a residue instead of 0; next to any non-zero V value it is far below one float64 ulp
    out = torch.where(out.abs() < 1e-60, torch.zeros_like(out), out)
    return dict(qkv=qkv, qb=qb, tab=tab, out=out, lse=lse, exact=(pmax == 1.0))


@functools.lru_cache(maxsize=None)
def routing_ref(case):
    _threads()
    return routing_ref_of(routing_inputs(case), case)


def random_inputs(case, dtype, per_sample):
    """qkv ~ 0.7 randn, bias 0.3 randn, table 0.3 randn, dout ~ randn, float64 values that the compute dtype holds exactly (the
    table stays fp32 in both dtypes: it is what the kernels take)"""
    (S, H, W), ws, shift, heads, hd, bws = CASES[case]
    C = heads * hd
    g = torch.Generator().manual_seed(200 + ord(case) + (50 if per_sample else 0))
    qkv, qb, dout = rnd(dtype, torch.randn(2, S, H, W, 3 * C, generator=g) * 0.7, torch.randn(3 * C, generator=g) * 0.3,
                        torch.randn(2, S, H, W, C, generator=g))
    tab = torch.randn(*((2,) if per_sample else ()), (2 * bws - 1) ** 3, heads, generator=g) * 0.3
    return qkv.double(), qb.double(), tab.double(), dout.double()


def random_ref_of(inputs, case, _variant=None):
    (S, H, W), ws, shift, heads, hd, bws = CASES[case]
    qkv, qb, tab, dout = inputs
    q = qkv.clone().requires_grad_(True)
    t = tab.clone().requires_grad_(True)
    out, lse, _ = window_attention_ref(q, qb, t, heads, ws, shift, bws, _variant=_variant)
    (out * dout).sum().backward()
    return dict(qkv=qkv, qb=qb, tab=tab, dout=dout, out=out.detach(), lse=lse.detach(), dqkv=q.grad, dtable=t.grad)


@functools.lru_cache(maxsize=None)
def random_ref(case, dtype, per_sample):
    _threads()
    return random_ref_of(random_inputs(case, dtype, per_sample), case)


# ------------------------------------------------------------------------------------------------------------------
# metrics
# ------------------------------------------------------------------------------------------------------------------
def to_windows(t, ws, shift):
    """[B,S,H,W,C] -> [B*nW, ws^3 * C] on the zero-padded, shifted grid (padding adds nothing to either norm)"""
    from oracle.swin import window_partition
    B, S, H, W, C = t.shape
    pad = [(-L) % ws for L in (S, H, W)]
    t = torch.nn.functional.pad(t, (0, 0, 0, pad[2], 0, pad[1], 0, pad[0]))
    if shift:
        t = torch.roll(t, shifts=(-shift, -shift, -shift), dims=(1, 2, 3))
    return window_partition(t, ws).reshape(-1, ws ** 3 * C)


def _rows_rel_l2(got, ref):
    den = ref.norm(dim=1)
    live = den > 0
    return float(((got - ref).norm(dim=1)[live] / den[live]).max())


def metrics(name, got, ref, ws, shift):
    """(max |err| / max |ref|, worst window) of one tensor against its float64 reference"""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, f"{name}: shape {tuple(got.shape)} vs reference {tuple(ref.shape)}"
    assert bool(torch.isfinite(got).all()), f"{name}: not finite"
    m1 = float((got - ref).abs().max() / ref.abs().max())
    if name == "dtable":          # per head column (per sample and head for per-sample tables)
        m2 = _rows_rel_l2(got.transpose(-1, -2).reshape(-1, ref.shape[-2]), ref.transpose(-1, -2).reshape(-1, ref.shape[-2]))
    elif name == "lse":           # [B*nW, heads, N]: one row per window already
        m2 = _rows_rel_l2(got.reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1))
    else:
        m2 = _rows_rel_l2(to_windows(got, ws, shift), to_windows(ref, ws, shift))
    return m1, m2


def gate(kernel, name, m, what):
    g = ATTN_GATES[kernel][name]
    print(f"  {what}: {name} [{kernel}] max-rel {m[0]:.3e} (gate {g[0]:.1e}), worst window {m[1]:.3e} (gate {g[1]:.1e})")
    return [] if m[0] <= g[0] and m[1] <= g[1] else [f"{name} [{kernel}]: max-rel {m[0]:.3e} / worst window {m[1]:.3e} "
                                                       f"over the gates {g[0]:.1e} / {g[1]:.1e}"]


# ------------------------------------------------------------------------------------------------------------------
# path selection
# ------------------------------------------------------------------------------------------------------------------
def _tier(N):
    nkt = (N + 31) // 32
    return 1 if nkt == 1 else 2 if nkt == 2 else 4 if nkt <= 4 else 7 if nkt <= 7 else 11


def route(case, path, per_sample, monkeypatch):
    """set the path's switches, then (forward kernel, backward kernel, tier): the backward from the library's workspace query,
    the forward and the tier from the dispatch rule of msseg_window_attention_fwd; fails if it is not the row's path"""
    from medicalsemseg_amd import hip
    (S, H, W), ws, shift, heads, hd, bws = CASES[case]
    dtype, env = PATHS[path]
    for k in ("MSSEG_ATTN_NO_MFMA", "MSSEG_ATTN_BWD_NO_WS"):
        monkeypatch.delenv(k, raising=False)
    if "MSSEG_ATTN_NO_MFMA" in env:
        monkeypatch.setenv("MSSEG_ATTN_NO_MFMA", "1")
    C, N, M3 = heads * hd, ws ** 3, (2 * bws - 1) ** 3
    stride = M3 * heads if per_sample else 0
    # without the no-workspace switch the query is non-zero exactly when the backward runs on the MFMA kernels
    wsb = int(hip.load_library().msseg_window_attention_bwd_workspace_bytes(2, S, H, W, C, heads, ws, shift, bws, stride,
                                                                            hip._DT[dtype]))
    no_ws = "MSSEG_ATTN_BWD_NO_WS" in env
    if no_ws:
        monkeypatch.setenv("MSSEG_ATTN_BWD_NO_WS", "1")
        assert int(hip.load_library().msseg_window_attention_bwd_workspace_bytes(2, S, H, W, C, heads, ws, shift, bws, stride,
                                                                                 hip._DT[dtype])) == 0
    name = "fp32" if dtype == F32 else "bf16"
    fwd_mfma = dtype == BF16 and hd in (16, 32) and N <= 352 and M3 <= 4095 and C % 8 == 0 and "MSSEG_ATTN_NO_MFMA" not in env
    fwd = "bf16_mfma" if fwd_mfma else name + "_vector"
    bwd = ("bf16_mfma_atomics" if no_ws else "bf16_mfma_ws") if wsb > 0 else name + "_vector"
    tier = _tier(N) if fwd_mfma else None
    print(f"case {case} {CASES[case]} path {path}{' per-sample tables' if per_sample else ''}: forward {fwd}"
          f"{f' NKT {tier}' if tier else ''}, backward {bwd} (workspace query {wsb} bytes)")
    assert (fwd, bwd, tier) == EXPECT[(case, path)], f"case {case} / {path} took {(fwd, bwd, tier)}, its row names {EXPECT[(case, path)]}"
    return fwd, bwd, tier


# ------------------------------------------------------------------------------------------------------------------
# (a) exact routing
# ------------------------------------------------------------------------------------------------------------------
def assert_routing_exact(got, ref, what):
    """got [B,S,H,W,C] == the float64 reference on every (token, head) row whose probability row is one-hot.  First, on the
    reference alone: the exact rows hold multiples of 1/8 with |v| <= 8 (exact in bf16) and are at least half of all rows."""
    out, exact = ref["out"], ref["exact"]
    B, S, H, W, heads = exact.shape
    hd = out.shape[-1] // heads
    share = float(exact.double().mean())
    assert share >= 0.5, f"{what}: only {share:.2f} of the (token, head) rows are exact: change the shape"
    o = out.reshape(B, S, H, W, heads, hd)
    sel = o[exact]
    assert bool((sel * 8 == (sel * 8).round()).all()) and float(sel.abs().max()) <= 8, f"{what}: exact rows are not multiples of 1/8 in [-8, 8]"
    g = got.detach().double().cpu().reshape(B, S, H, W, heads, hd)
    bad = ((g != o).any(-1) & exact).nonzero()
    if bad.shape[0] == 0:
        return share
    C = heads * hd
    msg = f"{what}: {bad.shape[0]} of {int(exact.sum())} exact (token, head) rows differ; first (b, z, y, x, head): "
    for i in bad[:4]:
        b, z, y, x, h = i.tolist()
        v = ref["qkv"][b, ..., 2 * C + h * hd:2 * C + (h + 1) * hd]              # [S, H, W, hd]
        hit = (v == g[b, z, y, x, h]).all(-1).nonzero()
        if hit.shape[0]:
            src = "the V row of voxel " + str(tuple(hit[0].tolist()))
        elif bool((ref["qb"][2 * C + h * hd:2 * C + (h + 1) * hd] == g[b, z, y, x, h]).all()):
            src = "the V row of a padded token (the bias)"
        else:
            src = "no single V row of this sample and head"
        want = (v == o[b, z, y, x, h]).all(-1).nonzero()
        msg += f"{(b, z, y, x, h)}: got {src}, want {'voxel ' + str(tuple(want[0].tolist())) if want.shape[0] else 'a padded token'}; "
    raise AssertionError(msg)


@pytest.mark.parametrize("case,path", FWD_RUNS)
def test_window_attention_routing_exact(monkeypatch, case, path):
    from medicalsemseg_amd import hip
    ref = routing_ref(case)                                   # CPU, before the first GPU call
    (S, H, W), ws, shift, heads, hd, bws = CASES[case]
    dtype, _ = PATHS[path]
    share = float(ref["exact"].double().mean())
    assert share >= 0.5, f"case {case}: only {share:.2f} of the (token, head) rows are exact: change the shape"
    fwd, _, _ = route(case, path, False, monkeypatch)
    qkv = ref["qkv"].to(DEV, dtype)
    assert torch.equal(qkv.double().cpu(), ref["qkv"])
    out = torch.full((2, S, H, W, heads * hd), float("nan"), device=DEV, dtype=dtype)
    hip.window_attention_fwd(qkv, ref["qb"].float().to(DEV), ref["tab"].float().to(DEV), out, heads, ws, shift, bws)
    torch.cuda.synchronize()
    print(f"  exact rows: {share:.3f} of all (token, head) rows; per head "
          f"{[round(float(ref['exact'][..., h].double().mean()), 2) for h in range(heads)]}")
    assert_routing_exact(out, ref, f"case {case} {path} ({fwd})")
    # the remaining rows are near-uniform averages: the gates of (b)
    fails = gate(fwd, "out", metrics("out", out, ref["out"], ws, shift), "routing data")
    assert not fails, fails


# ------------------------------------------------------------------------------------------------------------------
# (b) random data, forward and backward
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,path,per_sample", RANDOM_RUNS)
def test_window_attention_random_vs_float64(monkeypatch, case, path, per_sample):
    from medicalsemseg_amd import hip
    (S, H, W), ws, shift, heads, hd, bws = CASES[case]
    dtype, _ = PATHS[path]
    ref = random_ref(case, dtype, per_sample)                 # CPU, before the first GPU call
    fwd, bwd, _ = route(case, path, per_sample, monkeypatch)
    qkv, dout = ref["qkv"].to(DEV, dtype), ref["dout"].to(DEV, dtype)
    assert torch.equal(qkv.double().cpu(), ref["qkv"]) and torch.equal(dout.double().cpu(), ref["dout"])
    qb, tab = ref["qb"].float().to(DEV), ref["tab"].float().contiguous().to(DEV)
    out = torch.full((2, S, H, W, heads * hd), float("nan"), device=DEV, dtype=dtype)
    lse = hip.window_attention_fwd(qkv, qb, tab, out, heads, ws, shift, bws)
    dqkv = torch.full_like(qkv, float("nan"))
    dtab = torch.zeros_like(tab)
    hip.window_attention_bwd(qkv, qb, tab, out, lse, dout, dqkv, dtab, heads, ws, shift, bws)
    torch.cuda.synchronize()
    what = f"case {case} {path}"
    fails = []
    tab32 = ref["tab"].float().double()       # the reference saw the float64 image of the fp32 table
    assert torch.equal(tab32, ref["tab"])
    for kernel, name, got in ((fwd, "out", out), (fwd, "lse", lse), (bwd, "dqkv", dqkv), (bwd, "dtable", dtab)):
        fails += gate(kernel, name, metrics(name, got, ref[name], ws, shift), what)
    if (case, path, per_sample) in CALL_FORMS:
        d2 = torch.full_like(qkv, float("nan"))
        hip.window_attention_bwd(qkv, qb, tab, out, lse, dout, d2, None, heads, ws, shift, bws)
        same = torch.equal(d2, dqkv)
        d3 = torch.full_like(qkv, float("nan"))
        t3 = torch.full_like(tab, 0.5)
        hip.window_attention_bwd(qkv, qb, tab, out, lse, dout, d3, t3, heads, ws, shift, bws)
        torch.cuda.synchronize()
        print(f"  calling forms: dtable = None leaves dqkv bit-identical: {same}")
        assert same, f"{what}: dqkv differs between dtable = None and a dtable"
        assert torch.equal(d3, dqkv), f"{what}: dqkv differs with a pre-filled dtable"
        if bwd == "bf16_mfma_ws":            # fixed-order sums added to the buffer once: the same bits as 0.5 + gradient
            assert torch.equal(t3, dtab + 0.5), f"{what}: dtable pre-filled with 0.5 is not 0.5 + the gradient"
        fails += gate(bwd, "dtable", metrics("dtable", t3.double() - 0.5, ref["dtable"], ws, shift), what + ", dtable += onto 0.5")
    assert not fails, fails
