"""The fused AdamW step, the gradient-norm reduction and FlatAdamW against the float64 checker of tests/optim_ref.py, at the
sizes where the kernels change path (vector / scalar, one pass / grid-stride, one block / several / clipped to the partials
buffer), with every operand inside a sentinel-filled buffer.  The bounds are optim_ref's: derived from fp32 rounding and
shown on the CPU (tests/test_optim_host.py) to leave a correct fp32 implementation 2x head-room."""
import functools

import pytest
import torch

from tests import optim_ref as R
from tests.test_gpu_kernels import _dev

pytestmark = pytest.mark.gpu

SENTINEL = -32768.0
PAD = 64                       # sentinel floats (bytes for the mask) on either side: keeps the view 16-byte aligned
B1, B2, EPS = 0.9, 0.95, 1e-6
LRWD = {"test": (1e-2, 0.05), "production": (4e-4, 1e-5)}
T_ALL = (1, 2, 7, 1000, 100000)


def _num_cus():
    from medicalsemseg_amd import hip
    return hip.lib().msseg_num_cus()


class Guard1d:
    """a 1-D tensor in the middle of a sentinel-filled buffer, `lead` elements past the aligned position"""

    def __init__(self, src, dev, lead=0, sentinel=SENTINEL):
        n = src.numel()
        self.buf = torch.full((n + 2 * PAD + lead,), sentinel, dtype=src.dtype, device=dev)
        self.lo, self.hi = PAD + lead, PAD + lead + n
        self.t = self.buf[self.lo:self.hi]
        self.t.copy_(src)
        self.before = self.buf.clone()

    def assert_guard(self, what):
        assert torch.equal(self.buf[:self.lo], self.before[:self.lo]) and torch.equal(self.buf[self.hi:], self.before[self.hi:]), \
            f"{what}: wrote outside its tensor"

    def assert_unchanged(self, what):
        assert torch.equal(self.buf, self.before), f"{what}: an input was modified"


@functools.lru_cache(maxsize=4)
def _inputs(n, fresh):
    """(p, g, m, v) on the CPU, shared by the cases of one size: zero moments (fresh, t = 1) or random ones"""
    return R.make_inputs(n, 1 if fresh else 2)


@functools.lru_cache(maxsize=4)
def _mask(n):
    return R.random_mask(n)


def _run_adamw(n, lead, mask_kind, dev_path, gs, t, lrwd):
    from medicalsemseg_amd import hip
    dev = _dev()
    lr, wd = LRWD[lrwd]
    what = f"n={n} lead={lead} mask={mask_kind} {'device' if dev_path else 'host'} hyper gscale={gs} t={t} lr={lr} wd={wd}"
    p0, g0, m0, v0 = _inputs(n, t == 1)
    mask0 = None if mask_kind == "none" else _mask(n)
    gsv = 1.0 if gs is None else gs
    ref = R.adamw_step_f64(p0, g0, m0, v0, mask0, lr, B1, B2, EPS, wd, t, gsv)
    bnd = R.step_bounds(ref, m0, g0, lr, B1, B2, EPS, t, gsv)

    def launch(mask_cpu):
        p, g, m, v = (Guard1d(x, dev, lead) for x in (p0, g0, m0, v0))
        # an unaligned mask alone also sends the kernel down the scalar path: keep it aligned unless the floats are not
        mk = None if mask_cpu is None else Guard1d(mask_cpu, dev, lead, sentinel=7)
        gsc = None if gs is None else Guard1d(torch.tensor([gs]), dev)
        hyper = Guard1d(torch.tensor([lr, float(t)]), dev) if dev_path else None
        # with device hyper-parameters the host lr and step are deliberately wrong: the kernel must not use them
        hip.adamw_step(p.t, g.t, m.t, v.t, None if mk is None else mk.t, 123.0 if dev_path else lr, B1, B2, EPS, wd,
                       1 if dev_path else t, None if gsc is None else gsc.t, None if hyper is None else hyper.t)
        torch.cuda.synchronize()
        for x, name in ((p, "p"), (m, "m"), (v, "v")):
            x.assert_guard(f"{what}: {name}")
        for x, name in ((g, "g"), (mk, "mask"), (gsc, "gscale"), (hyper, "hyper")):
            if x is not None:
                x.assert_unchanged(f"{what}: {name}")
        return p.t.cpu(), m.t.cpu(), v.t.cpu()

    got = launch(mask0)
    for k, i in (("p", 0), ("m", 1), ("v", 2)):
        w = R.worst_ratio(got[i], ref[i], bnd[k])
        print(f"{what}: {k} error / bound {w:.3f}")
        assert w <= 1.0, f"{what}: {k} error is {w:.3f} of its bound"
    print(f"{what}: p error / bound without the propagated m term {R.worst_ratio(got[0], ref[0], bnd['p_issue']):.3f}")
    if lrwd == "production":
        # 1 - lr*wd is 1.0f: the same elements with no decay at all come back with the same bits
        undecayed = launch(torch.zeros(n, dtype=torch.uint8))
        assert torch.equal(got[0], undecayed[0]), f"{what}: decay changed a parameter at the production hyper-parameters"
        assert torch.equal(got[1], undecayed[1]) and torch.equal(got[2], undecayed[2])


# n, lead: 4 / 1028 vector; 1031 scalar (n % 4); 1028 one float into the buffers scalar (unaligned)
SMALL = [(4, 0), (1028, 0), (1031, 0), (1028, 1)]


@pytest.mark.parametrize("lrwd", ["test", "production"])
@pytest.mark.parametrize("gs", [None, 0.37])
@pytest.mark.parametrize("dev_path", [False, True], ids=["hosthyper", "devhyper"])
@pytest.mark.parametrize("mask_kind", ["none", "random"])
@pytest.mark.parametrize("n,lead", SMALL)
def test_adamw_step_small(n, lead, mask_kind, dev_path, gs, lrwd):
    for t in T_ALL:
        _run_adamw(n, lead, mask_kind, dev_path, gs, t, lrwd)


# the grid is capped at num_cus*16 blocks of 1024 elements: these sizes take a second, partial pass of the grid-stride loop
# (+1028: vector path, +1031: scalar path).  The cross product is thinned; every value of every axis appears for both.
BIG = [(1028, "none", False, None, 1, "test"), (1028, "random", True, 0.37, 2, "production"),
       (1028, "random", False, 0.37, 1000, "test"), (1028, "none", True, None, 100000, "production"),
       (1031, "random", True, None, 7, "test"), (1031, "none", False, 0.37, 2, "production"),
       (1031, "random", False, None, 1, "production"), (1031, "none", True, 0.37, 1000, "test")]


@pytest.mark.parametrize("extra,mask_kind,dev_path,gs,t,lrwd", BIG)
def test_adamw_step_grid_stride(extra, mask_kind, dev_path, gs, t, lrwd):
    _run_adamw(_num_cus() * 16 * 1024 + extra, 0, mask_kind, dev_path, gs, t, lrwd)


# ---- sumsq -------------------------------------------------------------------------------------------------------------
SUMSQ_N = [1, 255, 256, 257, 4097, 1_000_003]
PART_ROOM = 8192               # the partials view sits in front of this many floats: more than the kernel's largest grid


def _sumsq(x, n_partials):
    """-> (result, nblk); asserts that the partials beyond nblk, the floats after the partials view and around the result
    keep their sentinel"""
    from medicalsemseg_amd import hip
    dev = x.device
    n = x.numel()
    nblk = R.sumsq_nblk(n, _num_cus(), n_partials)
    assert _num_cus() * 16 <= PART_ROOM
    room = torch.full((PART_ROOM + 4096,), SENTINEL, device=dev)
    out = torch.full((3,), SENTINEL, device=dev)
    xg = Guard1d(x, dev)
    hip.sumsq(xg.t, out[1:2], room[:n_partials])
    torch.cuda.synchronize()
    xg.assert_unchanged("sumsq input")
    assert bool((room[nblk:] == SENTINEL).all()), f"sumsq n={n}: wrote partials beyond block {nblk} of {n_partials}"
    assert bool((room[:nblk] != SENTINEL).all())
    assert float(out[0]) == SENTINEL and float(out[2]) == SENTINEL
    return out[1].clone(), nblk


@pytest.mark.parametrize("n_partials", [1, 3, 4096])
@pytest.mark.parametrize("n", SUMSQ_N)
def test_sumsq_exact_on_integers(n, n_partials):
    """integers in [-3, 3], 9n < 2^24: every partial sum is an integer below 2^24, so any summation order is exact"""
    assert 9 * n < 2 ** 24
    gen = torch.Generator().manual_seed(n)
    x = torch.randint(-3, 4, (n,), generator=gen).float()
    want = float((x.double() ** 2).sum())
    a, _ = _sumsq(x.to(_dev()), n_partials)
    b, _ = _sumsq(x.to(_dev()), n_partials)
    assert float(a) == want, f"n={n} partials={n_partials}: {float(a)} != {want}"
    assert torch.equal(a, b)


@pytest.mark.parametrize("n_partials", [1, 3, 4096])
@pytest.mark.parametrize("n", SUMSQ_N)
def test_sumsq_random_within_tree_bound(n, n_partials):
    gen = torch.Generator().manual_seed(n + 7)
    x = torch.randn(n, generator=gen) * 10.0 ** (torch.rand(n, generator=gen) * 6 - 3)
    want = float((x.double() ** 2).sum())
    got, nblk = _sumsq(x.to(_dev()), n_partials)
    rel = abs(float(got.double()) - want) / want
    bound = 1.01 * R.sumsq_bound(n, nblk)
    print(f"sumsq n={n} nblk={nblk}: relative error {rel:.3e}, bound {bound:.3e}")
    assert rel <= bound


# ---- FlatAdamW ---------------------------------------------------------------------------------------------------------
SHAPES = [("w0", (5, 3)), ("s0", (3,)), ("aff.bias", (1, 3)), ("s1", (1,)), ("s2", (7,)), ("w1", (2, 2, 3, 3, 3)), ("s3", (6,))]
NO_DECAY = {"s0", "aff.bias", "s1", "s2", "s3"}      # the 1-D ones and the 2-D parameter whose name ends in .bias
LR0, LR1, WD = R.f32(1e-2), R.f32(4e-3), R.f32(0.05)
HB1, HB2, HEPS = R.f32(B1), R.f32(B2), R.f32(EPS)


def _module(dtype=torch.float32, seed=5):
    gen = torch.Generator().manual_seed(seed)
    net = torch.nn.Module()
    net.aff = torch.nn.Module()
    for name, shape in SHAPES:
        owner, leaf = (net.aff, name.split(".")[1]) if "." in name else (net, name)
        owner.register_parameter(leaf, torch.nn.Parameter(torch.randn(shape, generator=gen).to(dtype)))
    return net


def _grads(step, seed=0):
    """fixed fp32 gradients per parameter name; the norm is about 12 * scale: odd steps clip at max_norm 1, even ones do not"""
    gen = torch.Generator().manual_seed(100 * seed + step)
    scale = 0.5 if step % 2 else 0.02
    return {name: torch.randn(shape, generator=gen) * scale for name, shape in SHAPES}


def _flat(net, lr=LR0):
    from medicalsemseg_amd.optim import FlatAdamW, add_weight_decay
    return FlatAdamW(add_weight_decay(net, WD), lr=lr, betas=(HB1, HB2), eps=HEPS)


def _torch_adamw(net, lr=LR0):
    from medicalsemseg_amd.optim import add_weight_decay
    return torch.optim.AdamW(add_weight_decay(net, WD), lr=lr, betas=(HB1, HB2), eps=HEPS)


def _set_grads(net, gs, flat):
    for name, p in net.named_parameters():
        if flat:
            p.grad.copy_(gs[name])
        else:
            p.grad = gs[name].to(p.dtype).clone()


def _offsets(net, opt):
    """element offset of every parameter in the flat buffer, from the addresses of the views"""
    return {name: (p.data_ptr() - opt.flat_param.data_ptr()) // 4 for name, p in net.named_parameters()}


def _padding(net, opt):
    used = torch.zeros(opt.flat_param.numel(), dtype=torch.bool)
    for name, p in net.named_parameters():
        o = _offsets(net, opt)[name]
        assert not bool(used[o:o + p.numel()].any()), f"{name} overlaps another parameter"
        used[o:o + p.numel()] = True
    return ~used


def test_flat_adamw_layout():
    net = _module().to(_dev())
    opt = _flat(net)
    offs = _offsets(net, opt)
    want_mask = torch.zeros(opt.flat_param.numel(), dtype=torch.uint8)
    for name, p in net.named_parameters():
        assert p.grad.data_ptr() - opt.flat_grad.data_ptr() == 4 * offs[name]
        if p.ndim <= 1:
            assert offs[name] % 4 == 0, f"{name} starts at {offs[name]}"
        if name not in NO_DECAY:
            want_mask[offs[name]:offs[name] + p.numel()] = 1
    pad = _padding(net, opt)
    assert int(pad.sum()) > 3, "this parameter list is meant to leave padding slots in front of 1-D parameters"
    assert torch.equal(opt.decay_mask.cpu(), want_mask)
    for buf in (opt.flat_param, opt.flat_grad, opt.exp_avg, opt.exp_avg_sq, opt.decay_mask):
        assert buf.numel() % 4 == 0 and buf.numel() == opt.flat_param.numel()
    assert float(opt.flat_param.cpu()[pad].abs().max()) == 0.0


def _ref_norm(net64):
    return float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in net64.parameters())))


def _assert_params_within(net, net_ref, t, lr_max, what):
    for (name, p), q in zip(net.named_parameters(), net_ref.parameters()):
        w = R.worst_ratio(p.detach().cpu(), q.detach(), R.cumulative_bound(q.detach(), t, lr_max))
        assert w <= 1.0, f"{what}: {name} error is {w:.3f} of the cumulative bound after {t} steps"


def _norm_bound(opt):
    n = opt.flat_grad.numel()
    return 1.01 * R.sumsq_bound(n, R.sumsq_nblk(n, _num_cus(), 4096)) / 2


def test_flat_adamw_12_steps_against_float64_torch():
    dev = _dev()
    net, net64 = _module().to(dev), _module(torch.float64)
    opt, opt64 = _flat(net), _torch_adamw(net64)
    pad = _padding(net, opt)
    clipped = 0
    for t in range(1, 13):
        gs = _grads(t)
        _set_grads(net, gs, True)
        _set_grads(net64, gs, False)
        want = _ref_norm(net64)
        torch.nn.utils.clip_grad_norm_(net64.parameters(), 1.0)
        got = float(opt.clip_grad_norm_(1.0))
        assert abs(got - want) <= _norm_bound(opt) * want, f"step {t}: norm {got} vs {want}"
        clipped += want > 1.0
        if t == 5:
            for grp in opt.param_groups + opt64.param_groups:
                grp["lr"] = LR1
        opt.step(); opt64.step()
        opt.zero_grad(); opt64.zero_grad()
        _assert_params_within(net, net64, t, LR0, "12 steps")
        assert float(opt._gscale) == 1.0
    assert 0 < clipped < 12
    for buf, name in ((opt.flat_param, "flat_param"), (opt.exp_avg, "exp_avg"), (opt.exp_avg_sq, "exp_avg_sq")):
        assert float(buf.cpu()[pad].abs().max()) == 0.0, f"{name}: a padding slot moved"


def test_flat_adamw_world_averaging_scale():
    """the data-parallel wrapper halves _gscale before the clip (world of 2): norm and step are those of g / 2"""
    dev = _dev()
    net, net64 = _module().to(dev), _module(torch.float64)
    opt, opt64 = _flat(net), _torch_adamw(net64)
    for t in (1, 2, 3):
        gs = _grads(t + 1)                          # no clip, clip (the norm of g/2 is about 3), no clip
        _set_grads(net, gs, True)
        _set_grads(net64, {k: g / 2 for k, g in gs.items()}, False)
        want = _ref_norm(net64)
        torch.nn.utils.clip_grad_norm_(net64.parameters(), 1.0)
        opt._gscale.mul_(0.5)
        got = float(opt.clip_grad_norm_(1.0))
        assert abs(got - want) <= _norm_bound(opt) * want, f"step {t}: norm {got} vs {want}"
        opt.step(); opt64.step()
        _assert_params_within(net, net64, t, LR0, "world averaging")
        assert float(opt._gscale) == 1.0


def _clone_net(net, dev):
    twin = _module().to(dev)
    with torch.no_grad():
        for p, q in zip(twin.parameters(), net.parameters()):
            p.copy_(q.detach())
    return twin


def test_flat_adamw_state_dict_continuation_is_bit_equal():
    dev = _dev()
    net = _module().to(dev)
    opt = _flat(net)
    for t in range(1, 5):
        _set_grads(net, _grads(t), True)
        opt.clip_grad_norm_(1.0)
        if t == 3:
            for grp in opt.param_groups:
                grp["lr"] = LR1
        opt.step()
    twin = _clone_net(net, dev)
    opt2 = _flat(twin, lr=1e-3)                      # built with another lr: the loaded one has to take effect
    opt2.load_state_dict(opt.state_dict())
    for t in range(5, 8):
        for n_, o_ in ((net, opt), (twin, opt2)):
            _set_grads(n_, _grads(t), True)
            o_.clip_grad_norm_(1.0)
            o_.step()
    for (name, p), q in zip(net.named_parameters(), twin.parameters()):
        assert torch.equal(p, q), name
    assert torch.equal(opt.exp_avg, opt2.exp_avg) and torch.equal(opt.exp_avg_sq, opt2.exp_avg_sq)


def test_flat_adamw_continues_a_torch_adamw_state_dict():
    """4 steps of torch.optim.AdamW in fp32, its state dict loaded into FlatAdamW, 3 more steps on both"""
    dev = _dev()
    ref = _module()
    oref = _torch_adamw(ref)
    for t in range(1, 5):
        _set_grads(ref, _grads(t), False)
        oref.step()
    net = _clone_net(ref, dev)
    opt = _flat(net)
    opt.load_state_dict(oref.state_dict())
    assert opt._step == 4 and float(opt._hyper[1]) == 4.0
    for k, t in enumerate(range(5, 8), 1):
        _set_grads(ref, _grads(t), False)
        _set_grads(net, _grads(t), True)
        oref.step(); opt.step()
        _assert_params_within(net, ref, k, LR0, "torch state dict")
