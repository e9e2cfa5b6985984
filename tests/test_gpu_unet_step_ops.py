"""One real UNet training step, recorded call by call, and every `layers.py` call of it compared with a float64 reference
evaluated on THAT CALL'S OWN stored operands (teacher forcing: rounding does not compound, so every activation, gradient
tensor and parameter gradient of the bf16 step is gated at about one bf16 rounding / one fp32 summation error).  References
and gates: tests/unet_step_ref.py; why the whole-net comparisons cannot see what this sees: tests/test_unet_step_ref_host.py;
the design: DESIGN.md 2.3.

The recorder patches the methods of the op classes (and hip.maxpool2_bwd) for the duration of one step; product code is
untouched, and a recorded step gives the bits of a plain one (asserted)."""
import collections
import contextlib
import functools
import inspect
import os

import pytest
import torch

from tests import unet_step_ref as R
from tests.test_gpu_baseline import _blobs
from tests.test_gpu_conv_exact import launched

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# name: (features key, classes, compute dtype, batch, grid)
CASES = {
    "A": ("UNet", 3, torch.bfloat16, 2, (32, 32, 64)),
    # the split-K small-grid kernels (conv3d_k3_small.hip) take whole 3 x 6 x 6 tiles only: the smallest grid of this net with such a
    # level is 48^3 (12^3, 6^3 and the 3^3 special case below a 24^3 level); batch 2: the unit finish pairs the samples
    "C": ("UNet", 3, torch.bfloat16, 2, (48, 48, 48)),
    "B-bf16": ("UNetSmall", 2, torch.bfloat16, 1, (32, 32, 32)),
    "B-fp32": ("UNetSmall", 2, torch.float32, 1, (32, 32, 32)),
}

# kernel name -> (why shape A cannot select it, the existing test that checks the kernel against an independent reference).
# A name may stand here only if its selection provably needs more tiles than shape A has.
EXEMPT = {}


# ---- the recorder ------------------------------------------------------------------------------------------------------------
def _snap(v):
    if isinstance(v, torch.Tensor):
        return v.detach().clone()
    if isinstance(v, (tuple, list)):
        return type(v)(_snap(u) for u in v)
    return v            # hand-off tokens (APPLIED, HeadGrad, None), op objects, numbers: as they are


def _has_tensor(v):
    return isinstance(v, torch.Tensor) or (isinstance(v, (tuple, list)) and any(_has_tensor(u) for u in v))


class Record:
    def __init__(self, kind, obj, args):
        self.kind, self.obj, self.args = kind, obj, args
        self.ret, self.after, self.grads, self.nested = None, {}, {}, []


def _targets():
    from medicalsemseg_amd import hip, layers
    L = layers
    return [(L.ConvNormAct, "fwd"), (L.Conv3, "fwd"), (L.InstNormAct, "fwd"), (L.Deconv2, "fwd"), (L.Conv1, "fwd"),
            (L.Conv1, "fwd_norm"), (L.InstNormAct, "bwd"), (L.InstNormAct, "pool_bwd_reduce"), (L.Conv3, "bwd"),
            (L.Conv3, "bwd_stem_inbwd"), (L.Deconv2, "bwd"), (L.Conv1, "bwd"), (L.Conv1, "bwd_norm"), (hip, "maxpool2_bwd")]


@contextlib.contextmanager
def recording(net):
    """records every call of the step's op methods: tensor arguments cloned before the call, the return value cloned, the
    tensor arguments cloned again after it (outputs are views of concat buffers, accumulated in place), and the gradient of
    every parameter of `net` that the call was the first to write"""
    recs, stack, claimed = [], [], set()
    params = dict(net.named_parameters())

    def wrap(owner, name, orig):
        sig = inspect.signature(orig)
        method = inspect.isclass(owner)
        kind = f"{owner.__name__.rsplit('.', 1)[-1]}.{name}"

        @functools.wraps(orig)
        def w(*a, **k):
            ba = sig.bind(*a, **k)
            ba.apply_defaults()
            rec = Record(kind, a[0] if method else None, {n: _snap(v) for n, v in ba.arguments.items() if n != "self"})
            if stack:
                stack[-1].nested.append(kind)
            recs.append(rec)
            stack.append(rec)
            try:
                ret = orig(*a, **k)
            finally:
                stack.pop()
            rec.ret = _snap(ret)
            rec.after = {n: _snap(v) for n, v in ba.arguments.items() if n != "self" and _has_tensor(v)}
            for n, p in params.items():
                if p.grad is not None and n not in claimed:
                    claimed.add(n)
                    rec.grads[n] = p.grad.detach().clone()
            return ret
        return w

    saved = [(o, n, getattr(o, n)) for o, n in _targets()]
    try:
        for o, n, orig in saved:
            setattr(o, n, wrap(o, n, orig))
        yield recs
    finally:
        for o, n, orig in saved:
            setattr(o, n, orig)


# ---- one case: a plain step, then the same step recorded -----------------------------------------------------------------
def _step(net, crit, x, y):
    for p in net.parameters():
        p.grad = None
    out = net((x, None, None))
    crit(out, y).backward()
    torch.cuda.synchronize()
    return out.detach().clone(), {n: p.grad.detach().clone() for n, p in net.named_parameters()}


def _net_and_data(key, n_cls, dtype, batch, grid, seed=0):
    from medicalsemseg_amd.models.unet import UNET_FEATURES, UNet
    torch.manual_seed(seed)
    net = UNet(1, n_cls, UNET_FEATURES[key], compute_dtype=dtype)
    with torch.no_grad():        # the affine parameters away from (1, 0): a dropped gamma or beta shows
        for name, p in net.named_parameters():
            if ".N." in name:
                p.add_(0.2 * torch.randn_like(p))
    x = torch.randn(batch, 1, *grid, generator=torch.Generator().manual_seed(seed + 13))
    y = _blobs(batch, max(grid), n_cls, seed + 14)[:, :, :grid[0], :grid[1], :grid[2]].contiguous()
    assert all(bool((y[b] == c).any()) for b in range(batch) for c in range(n_cls)), "a class is missing from the labels"
    return net.to(DEV), x.to(DEV), y.to(DEV)


@functools.lru_cache(maxsize=None)
def run_case(name):
    from medicalsemseg_amd.losses import DiceCELoss
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    net, x, y = _net_and_data(*CASES[name])
    crit = DiceCELoss()
    with launched() as seen:
        plain = _step(net, crit, x, y)
    with recording(net) as recs:
        recorded = _step(net, crit, x, y)
    return net, plain, recorded, recs, seen.names


@pytest.mark.parametrize("case", list(CASES))
def test_recording_does_not_perturb_the_step(case):
    net, (out0, g0), (out1, g1), recs, _ = run_case(case)
    assert torch.equal(out0, out1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    assert all(getattr(o, n).__name__ == n and not hasattr(getattr(o, n), "__wrapped__") for o, n in _targets())   # restored
    assert len(recs) > 40


# ---- the checker -----------------------------------------------------------------------------------------------------------
class Checker:
    def __init__(self, net):
        self.net, self.T = net, net.compute_dtype
        self.rt = self.T if self.T == torch.bfloat16 else None      # fp32 mode: no intermediate is rounded
        self.pn = {id(p): n for n, p in net.named_parameters()}
        self.worst, self.gated, self.tokens, self.acts = {}, collections.Counter(), collections.Counter(), {}
        self.where = {}
        for lvl, (c0, c1) in enumerate(net._enc):
            for u, c in (("c0", c0), ("c1", c1)):
                self._name(c, f"encoder level {lvl} {u}")
        for j, (up, c0, c1) in enumerate(net._dec):
            self.where[id(up)] = f"decoder level {3 - j} up"
            for u, c in (("c0", c0), ("c1", c1)):
                self._name(c, f"decoder level {3 - j} {u}")
        self.where[id(net._final)] = "head"

    def _name(self, cna, s):
        self.where[id(cna)], self.where[id(cna.conv)], self.where[id(cna.norm)] = s, s + " conv", s + " norm"

    # operands
    def W(self, p):
        """a conv weight as the compute dtype holds it (the packed images, the head's (T) cast)"""
        return R.rnd(p.detach().double().cpu(), self.rt)

    @staticmethod
    def F(t):
        return None if t is None else t.detach().double().cpu()

    def norm_ops(self, nrm):
        return self.F(nrm.gamma), self.F(nrm.beta), nrm.slope, nrm.eps

    # comparisons
    def cmp(self, i, rec, name, got, r64, r32, stored, exclude=None, slack=None):
        what = f"record {i} {rec.kind} [{self.where.get(id(rec.obj), '-')}] {name}"
        r = R.gate(got, r64.reshape(got.shape), r32.reshape(got.shape), stored, what, exclude, slack)
        self.worst[rec.kind] = max(self.worst.get(rec.kind, 0.0), r)

    def grad(self, i, rec, p, r64=None, r32=None, zero=False, slack=None):
        name = self.pn[id(p)]
        assert name in rec.grads, f"record {i} {rec.kind} [{self.where.get(id(rec.obj), '-')}]: {name}.grad was not written by this call"
        self.gated[name] += 1
        if zero:
            assert not bool(rec.grads[name].any()), f"record {i} {rec.kind}: {name}.grad (a bias in front of InstanceNorm) is not exactly 0"
        else:
            self.cmp(i, rec, f"{name}.grad", rec.grads[name], r64, r32, torch.float32, slack=slack)

    def unit_sums(self, i, rec, nrm, yraw, stats, da_stored, red):
        """the receiving unit's sums, formed by a producer kernel from the gradient it stored: red, dgamma, dbeta"""
        g, b, sl, ep = self.norm_ops(nrm)
        r64, r32 = R.both(lambda y, s, d, g_, b_: R.norm_act_bwd(y, s, d, g_, b_, sl, ep)[1:], self.F(yraw), self.F(stats), self.F(da_stored), g, b)
        self.cmp(i, rec, "red", red, r64[0], r32[0], torch.float32)
        self.grad(i, rec, nrm.gamma, r64[1], r32[1])
        self.grad(i, rec, nrm.beta, r64[2], r32[2])

    def handoff(self, i, rec, ret, next_norm, dgrad, ops):
        """the forms an input gradient leaves Conv3.bwd / Deconv2.bwd in; dgrad(*ops) -> the plain input gradient"""
        if isinstance(ret, list):
            self.tokens["two halves"] += 1
            split = tuple(t.shape[-1] for t in ret)
            r64, r32 = R.both(lambda *o: [h for h in torch.split(dgrad(*o), split, -1)], *ops)
            for k in range(2):
                self.cmp(i, rec, f"dx half {k}", ret[k], r64[k], r32[k], self.T)
            return
        if isinstance(ret, torch.Tensor):
            r64, r32 = R.both(dgrad, *ops)
            return self.cmp(i, rec, "dx", ret, r64, r32, self.T)
        dx, red = ret
        nrm, yraw, stats, act = next_norm
        g, b, sl, ep = self.norm_ops(nrm)
        from medicalsemseg_amd.layers import APPLIED
        if red is APPLIED:
            # the tensor returned IS the receiving unit's dyraw, and its dgamma / dbeta were written by this call
            self.tokens["APPLIED"] += 1
            self.tokens["APPLIED from " + rec.kind.split(".")[0]] += 1
            yr, st = self.F(yraw), self.F(stats)
            r64, r32 = R.both(lambda y, s, g_, b_, *o: R.applied_unit_bwd(dgrad(*o), y, s, g_, b_, sl, ep, self.rt), yr, st, g, b, *ops)
            da64, da32 = R.both(dgrad, *ops)          # rounded by the finish kernel before the unit's backward
            slack = R.rounded_da_slack(da64, 4.0 * float((da32 - da64).abs().max()), yr, st, g, ep, self.rt)
            self.cmp(i, rec, "dyraw of the receiving unit", dx, r64[0], r32[0], self.T, R.sign_ambiguous(yr, st, g, b, ep), slack)
            # the same ties in the unit's sums: one ulp of da (times |xhat| for dgamma) per near-tie element of the channel
            near, ulp = R.near_tie(da64, 4.0 * float((da32 - da64).abs().max()), self.rt)
            xhat = R.norm_bwd_parts(yr, st, da64, g, b, sl, ep)[1]
            self.grad(i, rec, nrm.gamma, r64[2], r32[2], slack=(near * ulp * xhat.abs()).sum((0, 1, 2, 3)))
            self.grad(i, rec, nrm.beta, r64[3], r32[3], slack=(near * ulp).sum((0, 1, 2, 3)))
            return
        r64, r32 = R.both(dgrad, *ops)
        self.cmp(i, rec, "dx", dx, r64, r32, self.T)
        if red is None:
            self.tokens["no sums"] += 1
        else:
            self.tokens["tensor red"] += 1
            self.unit_sums(i, rec, nrm, yraw, stats, dx, red)

    # one function per record kind
    def ConvNormAct_fwd(self, i, rec):
        a, (x, y, stats, act) = rec.ret
        self.acts[id(rec.obj.norm)] = act
        if rec.nested:
            return                                   # Conv3.fwd + InstNormAct.fwd ran inside: their own records are checked
        cv, nm = rec.obj.conv, rec.obj.norm          # small-grid unit: one finish kernel wrote all of it
        self.cmp(i, rec, "yraw", y, *R.both(R.conv3_fwd, self.F(x), self.W(cv.w), self.F(cv.b)), self.T)
        self.cmp(i, rec, "stats", stats, *R.both(R.stats_of, self.F(y)), torch.float32)
        g, b, sl, ep = self.norm_ops(nm)
        self.cmp(i, rec, "act", a, *R.both(lambda y_, s_, g_, b_: R.norm_act_fwd(y_, s_, g_, b_, sl, ep), self.F(y), self.F(stats), g, b), self.T)
        if rec.args["pooled"] is not None:
            self.cmp(i, rec, "pooled", rec.after["pooled"], *R.both(R.maxpool, self.F(a)), self.T)
        if rec.args["out"] is not None:
            assert torch.equal(rec.after["out"], a)

    def Conv3_fwd(self, i, rec):
        cv = rec.obj
        y, stats = rec.ret if isinstance(rec.ret, tuple) else (rec.ret, None)
        self.cmp(i, rec, "yraw", y, *R.both(R.conv3_fwd, self.F(rec.args["x"]), self.W(cv.w), self.F(cv.b)), self.T)
        if stats is not None:
            self.cmp(i, rec, "stats", stats, *R.both(R.stats_of, self.F(y)), torch.float32)

    def InstNormAct_fwd(self, i, rec):
        assert rec.args["residual"] is None
        a, stats = rec.ret
        y = rec.args["y_raw"]
        self.acts[id(rec.obj)] = a
        if rec.args["stats"] is None:
            self.cmp(i, rec, "stats", stats, *R.both(R.stats_of, self.F(y)), torch.float32)
        g, b, sl, ep = self.norm_ops(rec.obj)
        self.cmp(i, rec, "act", a, *R.both(lambda y_, s_, g_, b_: R.norm_act_fwd(y_, s_, g_, b_, sl, ep), self.F(y), self.F(stats), g, b), self.T)
        if rec.args["pooled"] is not None:
            self.cmp(i, rec, "pooled", rec.after["pooled"], *R.both(R.maxpool, self.F(a)), self.T)
        if rec.args["out"] is not None:
            assert torch.equal(rec.after["out"], a)

    def Deconv2_fwd(self, i, rec):
        up = rec.obj
        y = rec.after["out"] if rec.args["out"] is not None else rec.ret
        self.cmp(i, rec, "y", y, *R.both(R.deconv_fwd, self.F(rec.args["x"]), self.W(up.w), self.F(up.b)), self.T)

    def Conv1_fwd(self, i, rec):
        hd = rec.obj
        y = rec.after["out"] if rec.args["out"] is not None else rec.ret
        self.cmp(i, rec, "logits", y, *R.both(R.head_fwd, self.F(rec.args["x"]), self.W(hd.w), self.F(hd.b)), self.T)

    def Conv1_fwd_norm(self, i, rec):
        hd = rec.obj
        g, b, sl, ep = self.norm_ops(rec.args["nrm"])
        r = R.both(lambda y, s, g_, b_, w, bb: R.head_fwd_norm(y, s, g_, b_, sl, ep, w, bb, self.rt),
                   self.F(rec.args["yraw"]), self.F(rec.args["stats"]), g, b, self.W(hd.w), self.F(hd.b))
        slack = R.head_fwd_norm_slack(self.F(rec.args["yraw"]), self.F(rec.args["stats"]), g, b, sl, ep, self.W(hd.w), self.rt)
        self.cmp(i, rec, "logits", rec.after["out"], *r, self.T, slack=slack)

    def Conv1_bwd_norm(self, i, rec):
        from medicalsemseg_amd.layers import HeadGrad
        hd, nrm = rec.obj, rec.args["nrm"]
        g, b, sl, ep = self.norm_ops(nrm)
        dl = rec.args["dy"][..., :hd.cout]
        assert not bool(rec.args["dy"][..., hd.cout:rec.args["dy_channels"]].any()), "the class gradient rows' padding is not zero"

        def f(y, s, g_, b_, dl_, w):
            act = R.rnd(R.norm_act_fwd(y, s, g_, b_, sl, ep), self.rt)
            da, dw, db = R.head_bwd(act, dl_, w, self.rt)
            return (da, dw, db) + tuple(R.norm_act_bwd(y, s, da, g_, b_, sl, ep)[1:])
        r64, r32 = R.both(f, self.F(rec.args["yraw"]), self.F(rec.args["stats"]), g, b, self.F(dl), self.W(hd.w))
        da, red = rec.ret
        if isinstance(da, HeadGrad):     # no input gradient exists: the unit's apply forms it again from these
            self.tokens["HeadGrad"] += 1
            assert da.cout == hd.cout and torch.equal(da.w, hd.w.detach()) and torch.equal(da.dl[..., :hd.cout], dl)
        else:
            self.cmp(i, rec, "da", da, r64[0], r32[0], self.T)
        self.cmp(i, rec, "red", red, r64[3], r32[3], torch.float32)
        self.grad(i, rec, hd.w, r64[1], r32[1])
        self.grad(i, rec, hd.b, r64[2], r32[2])
        self.grad(i, rec, nrm.gamma, r64[4], r32[4])
        self.grad(i, rec, nrm.beta, r64[5], r32[5])

    def Conv1_bwd(self, i, rec):
        hd = rec.obj
        dl = self.F(rec.args["dy"][..., :hd.cout])
        r64, r32 = R.both(lambda a_, d_, w: R.head_bwd(a_, d_, w, None)[1:], self.F(rec.args["x"]), dl, self.W(hd.w))
        self.grad(i, rec, hd.w, r64[0], r32[0])
        self.grad(i, rec, hd.b, r64[1], r32[1])
        if rec.ret is not None:
            self.handoff(i, rec, rec.ret, rec.args["next_norm"], lambda d_, w: d_ @ w.reshape(w.shape[0], -1), (dl, self.W(hd.w)))

    def InstNormAct_bwd(self, i, rec):
        from medicalsemseg_amd.layers import APPLIED, HeadGrad
        nrm, da, red = rec.obj, rec.args["da"], rec.args["red"]
        assert not rec.args["want_dres"]
        if red is APPLIED:
            assert torch.equal(rec.ret, da)
            return
        g, b, sl, ep = self.norm_ops(nrm)
        y, st = self.F(rec.args["y_raw"]), self.F(rec.args["stats"])
        ex = R.sign_ambiguous(y, st, g, b, ep)

        def apply(y_, s_, g_, b_, da_, red_):
            dz, xh, sc = R.norm_bwd_parts(y_, s_, da_, g_, b_, sl, ep)
            return R.norm_bwd_apply_parts(dz, xh, sc, red_)
        if isinstance(da, HeadGrad):
            r = R.both(lambda y_, s_, g_, b_, dl, w, red_: apply(y_, s_, g_, b_, R.head_da(dl, w, self.rt), red_),
                       y, st, g, b, self.F(da.dl[..., :da.cout]), R.rnd(self.F(da.w), self.rt), self.F(red))
            dl, w = self.F(da.dl[..., :da.cout]), R.rnd(self.F(da.w), self.rt).reshape(da.cout, -1)
            slack = R.rounded_da_slack(dl @ w, 8 * 2.0 ** -24 * (dl.abs() @ w.abs()), y, st, g, ep, self.rt)     # <= 4 products, fp32
            return self.cmp(i, rec, "dyraw (deferred head gradient)", rec.ret, *r, self.T, ex, slack)
        if red is not None:
            return self.cmp(i, rec, "dyraw", rec.ret, *R.both(apply, y, st, g, b, self.F(da), self.F(red)), self.T, ex)
        r64, r32 = R.both(lambda y_, s_, d_, g_, b_: R.norm_act_bwd(y_, s_, d_, g_, b_, sl, ep), y, st, self.F(da), g, b)
        self.cmp(i, rec, "dyraw", rec.ret, r64[0], r32[0], self.T, ex)
        self.grad(i, rec, nrm.gamma, r64[2], r32[2])
        self.grad(i, rec, nrm.beta, r64[3], r32[3])

    def InstNormAct_pool_bwd_reduce(self, i, rec):
        if rec.ret is None:
            self.tokens["pool_bwd_reduce None"] += 1
            return
        self.tokens["pool_bwd_reduce fused"] += 1
        da, red = rec.ret
        act = self.acts[id(rec.obj)]           # the STORED activation of this unit (the skip): ties go to its first maximum
        r = R.both(R.pool_skip_grad, self.F(act), self.F(rec.args["skip_grad"]), self.F(rec.args["pooled_grad"]))
        self.cmp(i, rec, "da = skip + pooled", da, *r, self.T)
        self.unit_sums(i, rec, rec.obj, rec.args["y_raw"], rec.args["stats"], da, red)

    def hip_maxpool2_bwd(self, i, rec):
        skip = self.F(rec.args["dx"]) if rec.args["accumulate"] else torch.zeros_like(self.F(rec.args["dx"]))
        r = R.both(R.pool_skip_grad, self.F(rec.args["x"]), skip, self.F(rec.args["dy"]))
        self.cmp(i, rec, "dx", rec.after["dx"], *r, self.T)

    def Conv3_bwd(self, i, rec):
        cv = rec.obj
        assert rec.args["dx_out"] is None and not rec.args["accumulate_dx"]
        x, dy = self.F(rec.args["x"]), self.F(rec.args["dy"])
        self.grad(i, rec, cv.w, *R.both(R.conv3_wgrad, x, dy))
        if rec.args["bias_grad_is_zero"]:
            self.grad(i, rec, cv.b, zero=True)
        else:
            self.grad(i, rec, cv.b, *R.both(R.channel_sum, dy))
        if rec.ret is not None:
            self.handoff(i, rec, rec.ret, rec.args["next_norm"], R.conv3_dgrad, (dy, self.W(cv.w)))

    def Conv3_bwd_stem_inbwd(self, i, rec):
        self.tokens["bwd_stem_inbwd"] += 1
        cv, a = rec.obj, rec.args
        g, b, sl, ep = self.norm_ops(a["norm"])
        r = R.both(lambda x, y, s, da, red, g_, b_: R.stem_wgrad(x, y, s, da, red, g_, b_, sl, ep, self.rt),
                   self.F(a["x"]), self.F(a["y_raw"]), self.F(a["stats"]), self.F(a["da"]), self.F(a["red"]), g, b)
        self.grad(i, rec, cv.w, *r)
        self.grad(i, rec, cv.b, zero=True)

    def Deconv2_bwd(self, i, rec):
        up = rec.obj
        x, dy, w = self.F(rec.args["x"]), self.F(rec.args["dy"]), self.W(up.w)
        r64, r32 = R.both(lambda x_, d_, w_: R.deconv_bwd(x_, d_, w_)[1:], x, dy, w)
        self.grad(i, rec, up.w, r64[0], r32[0])
        self.grad(i, rec, up.b, r64[1], r32[1])
        if rec.ret is not None:
            self.handoff(i, rec, rec.ret, rec.args["next_norm"], lambda d_, w_: torch.einsum("ndihjwko,coijk->ndhwc", R._children(d_), w_), (dy, w))

    def run(self, recs):
        for i, rec in enumerate(recs):
            getattr(self, rec.kind.replace(".", "_"))(i, rec)
        names = [n for n, _ in self.net.named_parameters()]
        wrong = {n: self.gated[n] for n in names if self.gated[n] != 1}
        assert not wrong, f"parameters not gated exactly once: {wrong}"
        return self.worst


@pytest.mark.parametrize("case", list(CASES))
def test_every_op_of_the_step_against_float64_on_its_own_operands(case):
    net, _, _, recs, _ = run_case(case)
    ck = Checker(net)
    try:
        worst = ck.run(recs)
    finally:
        print(f"\n[{case}] worst error / gate per record kind (reported, not gated): "
              + ", ".join(f"{k} {v:.3f}" for k, v in sorted(ck.worst.items())))
        print(f"[{case}] hand-off tokens: {dict(ck.tokens)}")
    assert worst and max(worst.values()) <= 1.0
    if case == "C":
        assert any(r.kind == "ConvNormAct.fwd" and not r.nested for r in recs), "no small-grid forward unit at 48^3"
        assert ck.tokens["APPLIED"] > ck.tokens["APPLIED from Deconv2"] >= 1, f"no small-grid conv finish unit at 48^3: {dict(ck.tokens)}"
    if case == "A":
        # every hand-off form of the benchmarked step occurs at shape A
        yraw = [r for r in recs if r.kind == "Conv1.fwd_norm"]
        assert yraw and net._final.head_norm_ok(yraw[0].args["yraw"])       # the fused head, hence a HeadGrad
        for tok in ("tensor red", "APPLIED", "HeadGrad", "two halves", "pool_bwd_reduce fused", "bwd_stem_inbwd"):
            assert ck.tokens[tok] >= 1, f"shape A never produced the hand-off '{tok}': {dict(ck.tokens)}"


def test_shapes_cover_the_kernels_of_the_benchmarked_step():
    """names(2 x 96^3 bf16 UNet base step) is a subset of names(A) | names(B) | names(C) | EXEMPT (msseg_ktimer_* launch records)"""
    from medicalsemseg_amd.losses import DiceCELoss
    small = set()
    for case in CASES:
        small |= run_case(case)[4]
    net, x, y = _net_and_data("UNet", 3, torch.bfloat16, 2, (96, 96, 96))
    with launched() as seen:
        _step(net, DiceCELoss(), x, y)
    print(f"\nkernels of the 2 x 96^3 step: {sorted(seen.names)}\nkernels of the recorded shapes: {sorted(small)}")
    missing = seen.names - small - set(EXEMPT)
    assert not missing, f"kernels of the benchmarked step that no recorded shape launches: {sorted(missing)}"
    assert not (set(EXEMPT) & small), f"exempt kernels that a recorded shape does launch: {sorted(set(EXEMPT) & small)}"
