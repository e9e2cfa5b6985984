"""Plain-torch CPU references of every mathematical op of one UNet training step (models/unet.py through layers.py), and
the gates a stored result is held to.  No HIP, no autograd: each function is the formula written out.

Conventions
    * tensors are channels-last [N, D, H, W, C] as the kernels store them; weights keep torch's layouts
      (Conv3d [Cout, Cin, 3, 3, 3], ConvTranspose3d [Cin, Cout, 2, 2, 2], the head [Cout, Cin, 1, 1, 1]);
    * every function computes in the dtype of its operands: the caller upcasts the recorded operands to float64 for the
      reference and to float32 for the summation-error term of the gates (`both`);
    * statistics are `stats[n, c] = (sum, sum of squares)` of the STORED raw conv output; an op that consumes statistics or
      the backward sums `red[n, c] = (sum dz, sum dz * xhat)` (unscaled: the apply pass divides by S, instnorm.hip:64-65) takes
      the recorded tensor and evaluates csrc/common.h `mean_rstd` (var = s2 / S - mean^2, clamped at 0) on it;
    * dgamma = sum_n red[n, c, 1], dbeta = sum_n red[n, c, 0] (instnorm.hip:552).

Intermediate roundings (`round_to`: the compute dtype, None = none).  These are all of them; results are NOT rounded here (the
stored result is compared under a gate that allows its one rounding):
    * weights of every conv / transposed conv / head are used as the compute dtype holds them: the packed images
      (hip.pack_conv_k3, pack_conv_gather, pack_deconv) and head_conv.hip:78,150,195 `(float)(T)w[i]`  -> `rnd(w, round_to)`
      by the caller, once, before any op;
    * the fused head recomputes the last unit's activation and rounds it as the forward would have stored it:
      head_conv.hip:227 (forward), head_conv.hip:98 (weight gradient)                            -> `head_fwd_norm`, `head_bwd`;
    * the head's input gradient is rounded before it enters the unit's backward, stored or not: common.h:198 `head_da`
      (used by head_conv.hip:91 and instnorm.hip:173, the deferred HeadGrad form)                -> `head_da`;
    * the small-grid finish rounds the summed input gradient before the receiving unit's backward: conv3d_k3_small.hip:396
                                                                                                 -> `applied_unit_bwd`;
    * the generic / ping-pong / transposed-conv input-gradient kernels form the receiving unit's sums from the value as stored:
      igemm_fwd_kernel.h:559, pingpong.h:142                       -> the caller passes the recorded (stored) gradient as `da`;
    * the pooled + skip kernel rounds the sum before its sums: instnorm.hip:449                  -> `pool_skip_grad` + caller;
    * the stem weight gradient rounds the dy it forms: stem_conv.hip (hip.conv3d_stem_wgrad_inbwd: "the bits of
      instnorm_act_bwd_apply into a tensor followed by conv3d_gather_wgrad")                     -> `stem_wgrad`.
"""
from __future__ import annotations

import torch

BF16_HALF_ULP = 2.0 ** -8      # bf16 has 8 significant bits: half an ulp is 2^-8 * 2^floor(log2 |x|) <= 2^-8 |x|
FP32_GATE = 2e-5               # tests/test_gpu_kernels.py::check, fp32
SIGN_EPS = 1e-5                # |z| <= SIGN_EPS * max |z|: the sign of the pre-activation is not decided in fp32
SIGN_FP32 = 64 * 2.0 ** -24    # ... and within the zone, only what fp32 rounding of scale and shift can really flip (sign_ambiguous)
SIGN_SHARE = 1e-4              # at most this share of a tensor may be excluded for it


def rnd(t, round_to):
    """t as the dtype `round_to` holds it, back in t's dtype (None: unchanged)"""
    if round_to is None or t is None or round_to == t.dtype:
        return t
    return t.to(round_to).to(t.dtype)


# ---- convolutions --------------------------------------------------------------------------------------------------------
def _pad1(x):
    return torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1, 1, 1))


def _taps():
    return [(a, b, c) for a in range(3) for b in range(3) for c in range(3)]


def conv3_fwd(x, w, b=None):
    """y[n, v, o] = b[o] + sum_{tap, i} x[n, v + tap - 1, i] * w[o, i, tap] (zero padding)"""
    N, D, H, W, _ = x.shape
    xp = _pad1(x)
    y = torch.zeros(N * D * H * W, w.shape[0], dtype=x.dtype)
    for a, b_, c in _taps():
        y += xp[:, a:a + D, b_:b_ + H, c:c + W].reshape(-1, x.shape[-1]) @ w[:, :, a, b_, c].t()
    y = y.reshape(N, D, H, W, -1)
    return y if b is None else y + b


def conv3_dgrad(dy, w, split=None):
    """dx[n, u, i] = sum_{tap, o} dy[n, u - tap + 1, o] * w[o, i, tap]; split = (ca, cb): the two channel halves as a list"""
    N, D, H, W, _ = dy.shape
    dxp = torch.zeros(N, D + 2, H + 2, W + 2, w.shape[1], dtype=dy.dtype)
    for a, b_, c in _taps():
        dxp[:, a:a + D, b_:b_ + H, c:c + W] += (dy.reshape(-1, dy.shape[-1]) @ w[:, :, a, b_, c]).reshape(N, D, H, W, -1)
    dx = dxp[:, 1:-1, 1:-1, 1:-1]
    if split is not None:
        return [dx[..., :split[0]], dx[..., split[0]:]]
    return dx


def conv3_wgrad(x, dy):
    """dw[o, i, tap] = sum_{n, v} dy[n, v, o] * x[n, v + tap - 1, i]"""
    N, D, H, W, cin = x.shape
    cout = dy.shape[-1]
    xp = _pad1(x)
    dw = torch.empty(cout, cin, 3, 3, 3, dtype=x.dtype)
    dyf = dy.reshape(-1, cout).t()
    for a, b_, c in _taps():
        dw[:, :, a, b_, c] = dyf @ xp[:, a:a + D, b_:b_ + H, c:c + W].reshape(-1, cin)
    return dw


def channel_sum(dy):
    return dy.reshape(-1, dy.shape[-1]).sum(0)


def deconv_fwd(x, w, b=None):
    """y[n, 2d+i, 2h+j, 2w+k, o] = b[o] + sum_c x[n, d, h, w, c] * w[c, o, i, j, k]"""
    N, D, H, W, _ = x.shape
    y = torch.einsum("ndhwc,coijk->ndihjwko", x, w).reshape(N, 2 * D, 2 * H, 2 * W, w.shape[1])
    return y if b is None else y + b


def _children(dy):
    N, D2, H2, W2, C = dy.shape
    return dy.reshape(N, D2 // 2, 2, H2 // 2, 2, W2 // 2, 2, C)


def deconv_bwd(x, dy, w):
    """(dx, dw, dbias) of the k2 s2 transposed conv"""
    d8 = _children(dy)
    dx = torch.einsum("ndihjwko,coijk->ndhwc", d8, w)
    dw = torch.einsum("ndhwc,ndihjwko->coijk", x, d8)
    return dx, dw, channel_sum(dy)


# ---- InstanceNorm + LeakyReLU ------------------------------------------------------------------------------------------------
def stats_of(y):
    """[N, C, 2] = (sum, sum of squares) over the voxels of the stored tensor"""
    f = y.reshape(y.shape[0], -1, y.shape[-1])
    return torch.stack([f.sum(1), (f * f).sum(1)], -1)


def mean_rstd(stats, S, eps):
    """csrc/common.h mean_rstd; [N, 1, 1, 1, C] each"""
    mean = stats[..., 0] / S
    var = (stats[..., 1] / S - mean * mean).clamp_min(0)
    sh = (stats.shape[0], 1, 1, 1, stats.shape[1])
    return mean.reshape(sh), ((var + eps) ** -0.5).reshape(sh)


def _S(y):
    return y.shape[1] * y.shape[2] * y.shape[3]


def preact(yraw, stats, gamma, beta, eps):
    """z = yraw * sc + sh with sc = rstd * gamma, sh = beta - mean * sc"""
    mean, rstd = mean_rstd(stats, _S(yraw), eps)
    sc = rstd * gamma
    return yraw * sc + (beta - mean * sc)


def lrelu(z, slope):
    return torch.where(z > 0, z, z * slope)


def norm_act_fwd(yraw, stats, gamma, beta, slope, eps):
    return lrelu(preact(yraw, stats, gamma, beta, eps), slope)


def maxpool(act):
    N, D, H, W, C = act.shape
    return act.reshape(N, D // 2, 2, H // 2, 2, W // 2, 2, C).amax((2, 4, 6))


def norm_bwd_parts(yraw, stats, da, gamma, beta, slope, eps, sign_from=None):
    """(dz, xhat, sc): dz = da where the pre-activation (or `sign_from`) is positive, else slope * da"""
    mean, rstd = mean_rstd(stats, _S(yraw), eps)
    z = preact(yraw, stats, gamma, beta, eps) if sign_from is None else sign_from
    dz = torch.where(z > 0, da, da * slope)
    return dz, (yraw - mean) * rstd, rstd * gamma


def norm_bwd_red(dz, xhat):
    """red[n, c] = (sum dz, sum dz * xhat) over the voxels"""
    N, C = dz.shape[0], dz.shape[-1]
    return torch.stack([dz.reshape(N, -1, C).sum(1), (dz * xhat).reshape(N, -1, C).sum(1)], -1)


def norm_bwd_apply_parts(dz, xhat, sc, red):
    S = _S(dz)
    sh = (red.shape[0], 1, 1, 1, red.shape[1])
    return sc * (dz - (red[..., 0] / S).reshape(sh) - xhat * (red[..., 1] / S).reshape(sh))


def norm_act_bwd(yraw, stats, da, gamma, beta, slope, eps, red=None):
    """(dyraw, red, dgamma, dbeta); red given (the recorded sums): the apply pass alone uses it, red / dgamma / dbeta returned
    are still this op's own sums of `da`"""
    dz, xhat, sc = norm_bwd_parts(yraw, stats, da, gamma, beta, slope, eps)
    own = norm_bwd_red(dz, xhat)
    dy = norm_bwd_apply_parts(dz, xhat, sc, own if red is None else red)
    return dy, own, own[..., 1].sum(0), own[..., 0].sum(0)


def sign_ambiguous(yraw, stats, gamma, beta, eps):
    """mask of the elements whose pre-activation is too close to 0 for fp32 to decide its sign, or None.

    The zone allowed is |z| <= SIGN_EPS * max |z|.  All of it cannot be left out under the SIGN_SHARE bound: the raw output is
    stored in bf16, so the values near the zero crossing of a (sample, channel) sit on a lattice coarser than the zone, a lattice
    point inside it carries many voxels at once, and the share of the full zone comes to 2e-5 ... 1.5e-4 per tensor of the
    recorded shapes (expected 2 * 1e-5 * max |z| * density at 0 = 5e-5).  Left out is the part of the zone in which fp32 really
    cannot decide: |z| <= SIGN_FP32 * (|y sc| + |mean sc| + |beta|).  mean, var = s2 / S - mean^2 and rsqrt in fp32 put a relative
    error of about (1 + 2 mean^2 / var) * 2^-23 on sc, so about 1.3e-6 of those terms on z for mean^2 / var up to 10;
    SIGN_FP32 = 64 * 2^-24 = 3.8e-6 leaves a factor 3 on that.  A tensor of fewer than 1 / SIGN_SHARE elements gets no exclusion:
    one element is already more than the share allowed."""
    if yraw.numel() * SIGN_SHARE < 1.0:
        return None
    mean, rstd = mean_rstd(stats, _S(yraw), eps)
    sc = rstd * gamma
    z = (yraw * sc + (beta - mean * sc)).abs()
    return (z <= SIGN_EPS * z.max()) & (z <= SIGN_FP32 * ((yraw * sc).abs() + (mean * sc).abs() + beta.abs()))


def applied_unit_bwd(da, yraw, stats, gamma, beta, slope, eps, round_to):
    """small-grid finish in unit mode: the summed input gradient `da` is rounded, then the receiving unit's whole backward"""
    return norm_act_bwd(yraw, stats, rnd(da, round_to), gamma, beta, slope, eps)


# ---- the 1x1x1 head ----------------------------------------------------------------------------------------------------------
def head_fwd(act, w, b):
    return act @ w.reshape(w.shape[0], -1).t() + b


def head_fwd_norm(yraw, stats, gamma, beta, slope, eps, w, b, round_to):
    return head_fwd(rnd(norm_act_fwd(yraw, stats, gamma, beta, slope, eps), round_to), w, b)


def head_da(dl, w, round_to):
    """input gradient of the head from the class gradient rows, rounded as the head's backward stores it"""
    return rnd(dl @ w.reshape(w.shape[0], -1), round_to)


def head_bwd(act, dl, w, round_to):
    """(da, dw, dbias); act: the head's input (stored, or recomputed and rounded by the caller)"""
    C = dl.shape[-1]
    dw = (dl.reshape(-1, C).t() @ act.reshape(-1, act.shape[-1])).reshape(w.shape)
    return head_da(dl, w, round_to), dw, channel_sum(dl)


# ---- pooled + skip gradient ----------------------------------------------------------------------------------------------
def maxpool_bwd(act, g, last=False):
    """g routed to the first (last=True: the last, a seeded error of the method test) maximum of each 2x2x2 cell of `act` in
    (d, h, w) scan order"""
    N, D, H, W, C = act.shape
    cells = act.reshape(N, D // 2, 2, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 7, 2, 4, 6).reshape(N, D // 2, H // 2, W // 2, C, 8)
    m = cells.amax(-1, keepdim=True)
    hit = (cells == m).to(torch.int8)
    idx = (7 - hit.flip(-1).argmax(-1)) if last else hit.argmax(-1)     # argmax of a 0/1 tensor: first 1
    one = torch.nn.functional.one_hot(idx, 8).to(g.dtype) * g.unsqueeze(-1)
    return one.reshape(N, D // 2, H // 2, W // 2, C, 2, 2, 2).permute(0, 1, 5, 2, 6, 3, 7, 4).reshape(N, D, H, W, C)


def pool_skip_grad(act, skip_grad, pooled_grad, last=False):
    return skip_grad + maxpool_bwd(act, pooled_grad, last)


# ---- stem weight gradient ------------------------------------------------------------------------------------------------
def stem_wgrad(x, yraw, stats, da, red, gamma, beta, slope, eps, round_to):
    dz, xhat, sc = norm_bwd_parts(yraw, stats, da, gamma, beta, slope, eps)
    return conv3_wgrad(x, rnd(norm_bwd_apply_parts(dz, xhat, sc, red), round_to))


# ---- intermediates that may round either way -------------------------------------------------------------------------------
# A value the kernel rounds to the compute dtype BEFORE using it (the list in the module docstring) is formed there in fp32.  Where
# its float64 value lies within the fp32 error of the midpoint between two neighbouring bf16 values, the kernel may hold the other
# neighbour: one ulp of that intermediate, times its weight in the result, is then no error of the kernel.  The functions below
# return that amount per element of the RESULT (zero wherever no intermediate is that close to a tie); `gate` adds it to the
# tolerance.  The closeness bounds come from the fp32 formulas, never from what a kernel returned.
def near_tie(v, err, round_to):
    """(mask of the elements of v within err of a rounding midpoint of `round_to`, spacing of bf16 at v)"""
    ulp = torch.pow(2.0, torch.floor(torch.log2(v.abs().clamp_min(1e-30))) - 7)
    if round_to is None:
        return torch.zeros_like(v, dtype=torch.bool), ulp
    return (0.5 * ulp - (v - rnd(v, round_to)).abs()) <= err, ulp


def head_fwd_norm_slack(yraw, stats, gamma, beta, slope, eps, w, round_to):
    """fused head forward: the recomputed activation (error of the pre-activation as in sign_ambiguous) times |w|"""
    mean, rstd = mean_rstd(stats, _S(yraw), eps)
    sc = rstd * gamma
    err = SIGN_FP32 * ((yraw * sc).abs() + (mean * sc).abs() + beta.abs())
    z = preact(yraw, stats, gamma, beta, eps)
    near, ulp = near_tie(lrelu(z, slope), torch.where(z > 0, err, err * slope), round_to)
    return (near * ulp) @ w.reshape(w.shape[0], -1).abs().t()


def rounded_da_slack(da, err, yraw, stats, gamma, eps, round_to):
    """a unit's backward apply fed with a gradient rounded on the way in: |sc| times one ulp of da where da is near a tie"""
    _, rstd = mean_rstd(stats, _S(yraw), eps)
    near, ulp = near_tie(da, err, round_to)
    return (rstd * gamma).abs() * ulp * near


# ---- gates -----------------------------------------------------------------------------------------------
def both(fn, *ops, **kw):
    """(fn on the operands as float64, fn on the operands as float32 upcast to float64); non-tensors pass through"""
    def cast(o, dt):
        if isinstance(o, torch.Tensor) and o.is_floating_point():
            return o.to(dt)
        if isinstance(o, (list, tuple)):
            return type(o)(cast(v, dt) for v in o)
        return o

    def up(r):
        if isinstance(r, torch.Tensor):
            return r.double()
        return type(r)(up(v) for v in r)
    r64 = fn(*cast(ops, torch.float64), **{k: cast(v, torch.float64) for k, v in kw.items()})
    r32 = fn(*cast(ops, torch.float32), **{k: cast(v, torch.float32) for k, v in kw.items()})
    return r64, up(r32)


def fp32_term(ref64, ref32):
    s = float(ref64.abs().max()) if ref64.numel() else 0.0
    return max(FP32_GATE * s, 4.0 * float((ref32 - ref64).abs().max()) if ref64.numel() else 0.0)


class GateError(AssertionError):
    pass


def gate(got, ref64, ref32, stored_dtype, what="", exclude=None, slack=None):
    """error / gate ratio (<= 1 passes) of a stored result; raises GateError with the worst element otherwise.
    stored_dtype float32: max |got - ref64| <= max(2e-5 s, 4 max |ref32 - ref64|); bfloat16: per element 2^-8 |ref64| on top.
    exclude: mask of sign-ambiguous elements (its share is asserted); slack: see "intermediates that may round either way"."""
    got = got.detach().double().cpu()
    assert tuple(got.shape) == tuple(ref64.shape), f"{what}: shape {tuple(got.shape)} vs {tuple(ref64.shape)}"
    t = fp32_term(ref64, ref32)
    tol = torch.full_like(ref64, t)
    if stored_dtype == torch.bfloat16:
        tol = tol + BF16_HALF_ULP * ref64.abs()
    if slack is not None:
        tol = tol + slack.reshape(tol.shape)
    err = (got - ref64).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    if exclude is not None:
        share = float(exclude.double().mean())
        assert share <= SIGN_SHARE, f"{what}: {share:.2e} of the elements are sign-ambiguous (allowed {SIGN_SHARE:.0e})"
        err = torch.where(exclude, torch.zeros_like(err), err)
    if t == 0.0:     # an all-zero reference: the result must be zero
        ratio = 0.0 if float(err.max()) == 0.0 else float("inf")
        i = int(err.argmax())
    else:
        r = err / tol
        i = int(r.argmax())
        ratio = float(r.flatten()[i])
    if not ratio <= 1.0:
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref64.shape)) if ref64.dim() else ()
        raise GateError(f"{what}: error / gate = {ratio:.3g} at index {idx}: got {float(got.flatten()[i])!r} want "
                        f"{float(ref64.flatten()[i])!r} (gate {float(tol.flatten()[i]):.3e}, fp32 term {t:.3e}, "
                        f"{int((err > tol).sum())} of {err.numel()} elements over)")
    return ratio


# ---- the whole step chained from the ops above (host test: reference correctness and the seeded-error method) -------------
def unit_names():
    enc = ["conv_0", "down_1.convs", "down_2.convs", "down_3.convs", "down_4.convs"]
    dec = ["upcat_4", "upcat_3", "upcat_2", "upcat_1"]
    return enc, dec


class Step:
    """One UNet training step on the CPU through the reference ops.  `store`: dtype the activations / gradients are held in
    between ops (None: float64 throughout, no rounding anywhere).  Every op goes through `call`, which logs
    (kind, where, fn, operands, output kinds, stored outputs) and lets `tamper(kind, where, operands, outputs)` replace the
    outputs of one op before they are stored: the seeded errors of the method test."""

    def __init__(self, params, slope=0.1, eps=1e-5, store=None, tamper=None):
        self.store, self.tamper, self.slope, self.eps = store, tamper, slope, eps
        self.p = {k: (rnd(v.double(), store) if k.endswith("weight") and v.dim() == 5 else v.double()) for k, v in params.items()}
        self.grads, self.log = {}, []

    def call(self, kind, where, fn, ops, kinds):
        outs = fn(*ops)
        outs = list(outs) if isinstance(outs, (tuple, list)) else [outs]
        if self.tamper is not None:
            outs = list(self.tamper(kind, where, ops, outs) or outs)
        stored = [rnd(o, self.store) if k == "T" else (o.float().double() if self.store is not None else o)
                  for o, k in zip(outs, kinds)]
        self.log.append((kind, where, fn, ops, kinds, stored))
        return stored if len(stored) > 1 else stored[0]

    def _unit_fwd(self, name, x):
        P, sl, ep = self.p, self.slope, self.eps
        y = self.call("conv3_fwd", name, conv3_fwd, (x, P[name + ".conv.weight"], P[name + ".conv.bias"]), "T")
        st = self.call("stats", name, stats_of, (y,), "f")
        a = self.call("norm_act_fwd", name, lambda y_, s_, g_, b_: norm_act_fwd(y_, s_, g_, b_, sl, ep),
                      (y, st, P[name + ".adn.N.weight"], P[name + ".adn.N.bias"]), "T")
        return a, (x, y, st, a)

    def _unit_bwd(self, name, saved, da, need_dx=True, split=None):
        P, G, sl, ep = self.p, self.grads, self.slope, self.eps
        x, y, st, a = saved
        dy, red, dg, db = self.call("norm_act_bwd", name, lambda y_, s_, d_, g_, b_: norm_act_bwd(y_, s_, d_, g_, b_, sl, ep),
                                    (y, st, da, P[name + ".adn.N.weight"], P[name + ".adn.N.bias"]), "Tfff")
        G[name + ".adn.N.weight"], G[name + ".adn.N.bias"] = dg, db
        G[name + ".conv.weight"] = self.call("conv3_wgrad", name, conv3_wgrad, (x, dy), "f")
        G[name + ".conv.bias"] = self.call("channel_sum", name, channel_sum, (dy,), "f")
        if not need_dx:
            return None
        if split is not None:
            return self.call("conv3_dgrad_split", name, lambda d_, w_: conv3_dgrad(d_, w_, split), (dy, P[name + ".conv.weight"]), "TT")
        return self.call("conv3_dgrad", name, conv3_dgrad, (dy, P[name + ".conv.weight"]), "T")

    def forward(self, x):
        """x [N, D, H, W, 1] -> logits [N, D, H, W, classes]"""
        P = self.p
        enc, dec = unit_names()
        self.sv = {}
        cur = rnd(x.double(), self.store)
        skips = []
        for lvl, nm in enumerate(enc):
            a0, self.sv[nm + ".conv_0"] = self._unit_fwd(nm + ".conv_0", cur)
            a1, self.sv[nm + ".conv_1"] = self._unit_fwd(nm + ".conv_1", a0)
            skips.append(a1)
            cur = self.call("maxpool", nm, maxpool, (a1,), "T") if lvl < 4 else a1
        for j, nm in enumerate(dec):
            lvl = 3 - j
            self.sv[nm + ".up_in"] = cur
            up = self.call("deconv_fwd", nm, deconv_fwd, (cur, P[nm + ".upsample.deconv.weight"], P[nm + ".upsample.deconv.bias"]), "T")
            a0, self.sv[nm + ".convs.conv_0"] = self._unit_fwd(nm + ".convs.conv_0", torch.cat([skips[lvl], up], -1))
            cur, self.sv[nm + ".convs.conv_1"] = self._unit_fwd(nm + ".convs.conv_1", a0)
        self.sv["head_in"] = cur
        self.skips = skips
        return self.call("head_fwd", "final_conv", head_fwd, (cur, P["final_conv.weight"], P["final_conv.bias"]), "T")

    def backward(self, dl):
        P, G, st = self.p, self.grads, self.store
        enc, dec = unit_names()
        dl = rnd(dl.double(), st)
        g, G["final_conv.weight"], G["final_conv.bias"] = self.call(
            "head_bwd", "final_conv", lambda a_, d_, w_: head_bwd(a_, d_, w_, st), (self.sv["head_in"], dl, P["final_conv.weight"]), "Tff")
        skip_grads = [None] * 4
        for j in range(3, -1, -1):
            nm, lvl = dec[j], 3 - j
            g = self._unit_bwd(nm + ".convs.conv_1", self.sv[nm + ".convs.conv_1"], g)
            cs = self.skips[lvl].shape[-1]
            cat_c = self.sv[nm + ".convs.conv_0"][0].shape[-1]
            skip_grads[lvl], dup = self._unit_bwd(nm + ".convs.conv_0", self.sv[nm + ".convs.conv_0"], g, split=(cs, cat_c - cs))
            g, G[nm + ".upsample.deconv.weight"], G[nm + ".upsample.deconv.bias"] = self.call(
                "deconv_bwd", nm, deconv_bwd, (self.sv[nm + ".up_in"], dup, P[nm + ".upsample.deconv.weight"]), "Tff")
        for lvl in (4, 3, 2, 1, 0):
            nm = enc[lvl]
            if lvl < 4:
                g = self.call("pool_skip_grad", nm, pool_skip_grad, (self.skips[lvl], skip_grads[lvl], g), "T")
            g = self._unit_bwd(nm + ".conv_1", self.sv[nm + ".conv_1"], g)
            g = self._unit_bwd(nm + ".conv_0", self.sv[nm + ".conv_0"], g, need_dx=lvl > 0)
        return G

    def check(self, first=0):
        """every logged op (from entry `first`) against float64 on its own stored operands, under the gates;
        {kind: worst error / gate}"""
        worst = {}
        sdt = self.store if self.store is not None else torch.float32
        for i, (kind, where, fn, ops, kinds, stored) in enumerate(self.log):
            if i < first:
                continue
            r64, r32 = both(fn, *ops)
            r64 = list(r64) if isinstance(r64, (tuple, list)) else [r64]
            r32 = list(r32) if isinstance(r32, (tuple, list)) else [r32]
            for k, (got, a, b) in enumerate(zip(stored, r64, r32)):
                ex = None
                if kind == "norm_act_bwd" and k == 0:
                    ex = sign_ambiguous(ops[0], ops[1], ops[3], ops[4], self.eps)
                r = gate(got, a, b, sdt if kinds[k] == "T" else torch.float32, f"op {i} {kind} at {where}, output {k}", ex)
                worst[kind] = max(worst.get(kind, 0.0), r)
        return worst
