"""The fused Adam / AdamW + EMA launch (``oss_adam_ema_kernel`` and ``oss_adam_tick_kernel``, vmambair_amd/csrc/oss_optim.hip)
against a plain float64 step, per element and per quantity.

* The float64 step (``ref_step``) is pinned to ``torch.optim.Adam`` / ``AdamW`` run in float64 on the CPU (no GPU needed).
* Kernel level: the C ABI is driven directly with a hand-built chunk table.  Every array is a view at a chosen element
  offset into a sentinel-filled buffer, so the 16-byte path, the per-element path and what either writes next to its
  chunk are all seen.
* Class level: ``FusedAdamEMA`` over gradients that live in a ``ddp.FlatGrads`` buffer (misaligned views, as in the
  captured training step): a 64-step trajectory, resume from a state dict, and replay from a captured graph.

Tolerances are either the bounds below, which follow from the number of fp32 roundings in the kernel, or 4x the error of
torch's own fp32 Adam(W) on the CPU against the same float64 step, computed inside the test.

Every hyper-parameter is the value the kernel receives, ``float(np.float32(x))``: the C ABI takes ``float``.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from vmambair_amd import _capi

gpu = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 1234.5
PAD = 8            # sentinel elements in front of every view (a multiple of 4: the offset alone decides the alignment)


def f32(x):
    return float(np.float32(x))


def _hyper(b1, b2, wd, adamw):
    return dict(b1=f32(b1), b2=f32(b2), eps=f32(1e-8), wd=f32(wd), ema_decay=f32(0.999), adamw=adamw)


# the two steps of the trainings this project mirrors: SRGAN (Adam + EMA) and Deraining (AdamW + gradient clipping)
HYPER = {"srgan": _hyper(0.9, 0.99, 0.0, False), "deraining": _hyper(0.9, 0.999, 1e-4, True)}
LR = f32(2e-2)     # large on purpose: the update is ~1e5 ulp of p, so a 1e-4 relative error of the update shows


# ---- the float64 step --------------------------------------------------------------------------------------------------

def ref_step(p, m, v, ema, g, t, lr, b1, b2, eps, wd, ema_decay, grad_scale, bc1=None, bc2=None):
    """One Adam / AdamW + EMA step in float64 (NumPy), torch's formulas: decoupled decay first, ``exp_avg.lerp_``,
    ``exp_avg_sq``, ``denom = sqrt(v) / sqrt(bc2) + eps``, ``p -= lr / bc1 * m / denom``, then the EMA of the new p.
    ``t`` is the step being taken (1 for the first); ``bc1`` / ``bc2`` default to ``1 - beta^t`` in double."""
    bc1 = 1.0 - b1 ** t if bc1 is None else bc1
    bc2 = 1.0 - b2 ** t if bc2 is None else bc2
    g = g * grad_scale
    p = p * (1.0 - lr * wd)
    m = m + (g - m) * (1.0 - b1)
    v = b2 * v + (1.0 - b2) * g * g
    denom = np.sqrt(v) / np.sqrt(bc2) + eps
    p = p - (lr / bc1) * (m / denom)
    ema = None if ema is None else ema_decay * ema + (1.0 - ema_decay) * p
    return p, m, v, ema


def _gradients(rng, n):
    """magnitudes log-uniform in [1e-6, 1e2], random sign, about 5 % exact zeros; fp32 values"""
    g = 10.0 ** rng.uniform(-6.0, 2.0, n) * rng.choice([-1.0, 1.0], n)
    g[rng.random(n) < 0.05] = 0.0
    return g.astype(np.float32)


@pytest.mark.parametrize("adamw", [False, True], ids=["adam", "adamw"])
@pytest.mark.parametrize("name", sorted(HYPER))
def test_float64_step_reproduces_torch_in_double(name, adamw):
    """``ref_step`` with double bias corrections is ``torch.optim.Adam`` / ``AdamW`` (float64, CPU, foreach=False): 64 steps,
    parameters and both moments to 1e-12 relative, element by element."""
    hp = HYPER[name]
    wd = hp["wd"] if adamw else 0.0
    rng = np.random.default_rng(11)
    n = 777
    p = rng.standard_normal(n)
    m, v = np.zeros(n), np.zeros(n)
    q = torch.from_numpy(p.copy())
    cls = torch.optim.AdamW if adamw else torch.optim.Adam
    opt = cls([q], lr=LR, betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=wd, foreach=False)
    for t in range(1, 65):
        g = _gradients(rng, n).astype(np.float64)
        scale = 0.3 if t % 3 == 0 else 1.0
        q.grad = torch.from_numpy(g * scale)
        opt.step()
        p, m, v, _ = ref_step(p, m, v, None, g, t, LR, hp["b1"], hp["b2"], hp["eps"], wd, 0.0, scale)
    st = opt.state[q]
    assert float(st["step"]) == 64
    for what, got, want in (("p", p, q.numpy()), ("exp_avg", m, st["exp_avg"].numpy()), ("exp_avg_sq", v, st["exp_avg_sq"].numpy())):
        err = np.abs(got - want)
        assert (err <= 1e-12 * np.abs(want)).all(), (what, float(err.max()))


# ---- driving the C ABI -------------------------------------------------------------------------------------------------

class Slab:
    """``values`` (fp32) as a view ``off`` elements past a 16-byte boundary of a sentinel-filled device buffer, with at
    least 8 sentinel elements on either side"""

    def __init__(self, values, off):
        n = len(values)
        self.buf = torch.full((n + PAD + 16,), SENTINEL, dtype=torch.float32, device=DEV)
        assert self.buf.data_ptr() % 16 == 0 and 0 <= off <= 8
        self.lo, self.hi = PAD + off, PAD + off + n
        self.view = self.buf[self.lo:self.hi]
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)))
        self.before = self.buf.clone()

    def ptr(self):
        return self.buf.data_ptr() + 4 * self.lo

    def get(self):
        return self.view.cpu().numpy().astype(np.float64)

    def guards_intact(self):
        return (torch.equal(self.buf[:self.lo], self.before[:self.lo]) and
                torch.equal(self.buf[self.hi:], self.before[self.hi:]))

    def untouched(self):
        return torch.equal(self.buf, self.before)


def _rows(ptrs, n):
    """chunk-table rows of one tensor, as FusedAdamEMA._build lays them out (0 = NULL)"""
    rows = []
    for off in range(0, n, _capi.ADAM_CHUNK):
        b = 4 * off
        rows.append(tuple(q + b if q else 0 for q in ptrs) + (min(_capi.ADAM_CHUNK, n - off), 0))
    return rows


def _device_table(rows):
    arr = (_capi.AdamChunk * len(rows))(*[_capi.AdamChunk(*r) for r in rows])
    host = torch.empty(C.sizeof(arr), dtype=torch.uint8)
    C.memmove(host.data_ptr(), C.addressof(arr), C.sizeof(arr))
    return host.to(DEV)


def _launch(slabs, state, hp, lr_arg=-1.0, entry="adamw", scale=None, wd=None, table="build", n_chunks=None, null_state=False):
    """one call of the C ABI on the five slabs (``slabs['e']`` may be None = no EMA); returns the return code"""
    lib = _capi.load()
    n = slabs["p"].hi - slabs["p"].lo
    rows = _rows([slabs[k].ptr() if slabs[k] is not None else 0 for k in "pgmve"], n)
    tab = _device_table(rows)
    tab_ptr = tab.data_ptr() if table == "build" else None
    n_chunks = len(rows) if n_chunks is None else n_chunks
    st = None if null_state else state.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    if entry == "adam":
        rc = lib.oss_adam_ema_step(tab_ptr, n_chunks, st, lr_arg, hp["b1"], hp["b2"], hp["eps"], hp["ema_decay"], stream)
    else:
        rc = lib.oss_adamw_ema_step(tab_ptr, n_chunks, st, lr_arg, hp["b1"], hp["b2"], hp["eps"], hp["wd"] if wd is None else wd,
                                    hp["ema_decay"], scale.data_ptr() if scale is not None else None, stream)
    torch.cuda.synchronize()
    return rc


def _problem(n, t0, hp, seed, grad_scale):
    """a state after min(t0, 5) float64 warm-up steps (moments rounded to fp32; zeros for t0 = 0) and the next gradient"""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    ema = (p + 0.1 * rng.standard_normal(n)).astype(np.float32)
    m, v = np.zeros(n), np.zeros(n)
    for _ in range(min(t0, 5)):
        _, m, v, _ = ref_step(np.zeros(n), m, v, None, _gradients(rng, n).astype(np.float64), 1, 0.0, hp["b1"], hp["b2"],
                              hp["eps"], 0.0, 0.0, grad_scale)
    return dict(p=p, g=_gradients(rng, n), m=m.astype(np.float32), v=v.astype(np.float32), e=ema)


def _state(t0, lr=LR):
    # the two correction slots hold NaN: the tick has to overwrite them before the update reads them
    return torch.tensor([float(t0), float("nan"), float("nan"), lr], dtype=torch.float32, device=DEV)


def ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def one_step_bounds(x, ref, hp, lr, wd, s):
    """What a correct fp32 kernel may differ by from the float64 step after ONE step from fp32 inputs ``x``; each is a
    handful of fp32 roundings (units of 2^-24 relative):
    p    keep = fl(1 - lr wd), fl(p keep) and the final subtraction: 1.5 ulp of the larger of p and p'; the update
         lr / bc1 * m / (sqrt(v) rsqrt(bc2) + eps) carries ~11 units (3 of m, 2.5 of sqrt(v'), one per operation): 2^-20
    m    fl(g s), fl((1 - b1) gs), one fma: 3 units of |b1 m| + |(1 - b1) g s|: 2^-22
    v    gs twice, two products, one fma: 5 units of v': 2^-21
    ema  fl((1 - d) p'), one fma: 2 units of |ema| + |p'| (plus (1 - d) times the error of p'): 2^-22"""
    p, g, m, e = (x[k].astype(np.float64) for k in "pgme")
    pr, mr, vr, er = ref
    keep = 1.0 - lr * wd
    return dict(p=1.5 * ulp32(np.maximum(np.abs(p), np.abs(pr))) + 2.0 ** -20 * np.abs(pr - keep * p),
                m=2.0 ** -22 * (np.abs(hp["b1"] * m) + np.abs((1.0 - hp["b1"]) * g * s)),
                v=2.0 ** -21 * vr,
                e=None if er is None else 2.0 ** -22 * (np.abs(e) + np.abs(pr)))


def _check_one_step(slabs, x, state_after, hp, lr, wd, s, what):
    """the four results against the float64 step fed with the corrections the tick kernel left in ``state``"""
    has_ema = slabs["e"] is not None
    ref = ref_step(*(x[k].astype(np.float64) for k in "pmv"), x["e"].astype(np.float64) if has_ema else None,
                   x["g"].astype(np.float64), None, lr, hp["b1"], hp["b2"], hp["eps"], wd, hp["ema_decay"], s,
                   bc1=float(state_after[1]), bc2=float(state_after[2]))
    lim = one_step_bounds(x, ref, hp, lr, wd, s)
    worst = {}
    for k, r in zip("pmve", ref):
        if r is None:
            continue
        got = slabs[k].get()
        assert np.isfinite(got).all(), (what, k)
        err = np.abs(got - r)
        worst[k] = float(np.max(np.where(err > 0, err / np.maximum(lim[k], 1e-300), 0.0)))
    print(f"[one step {what}] error / bound: " + ", ".join(f"{k} {w:.3f}" for k, w in worst.items()))
    assert all(w <= 1.0 for w in worst.values()), (what, worst)
    return ref


def _slabs(x, offs=(0, 0, 0, 0, 0)):
    return {k: (Slab(x[k], o) if o is not None else None) for k, o in zip("pgmve", offs)}


T0S = (0, 1, 2, 9, 999, 69999)
GS_ONE_STEP = {"srgan": None, "deraining": f32(0.3)}   # not a power of two: fl(g s) rounds


@functools.lru_cache(maxsize=None)
def _one_step_run(name, t0):
    """ONE launch from a known state, shared by the per-element test and the tick test"""
    hp, s = HYPER[name], GS_ONE_STEP[name]
    n = 3001                                   # two chunks; the second ends in a 1-element tail
    x = _problem(n, t0, hp, 100 + t0, s or 1.0)
    slabs, state = _slabs(x), _state(t0)
    scale = None if s is None else torch.tensor([s], dtype=torch.float32, device=DEV)
    rc = _launch(slabs, state, hp, scale=scale)
    return rc, slabs, x, state.cpu().numpy()


@gpu
@pytest.mark.parametrize("t0", T0S)
@pytest.mark.parametrize("name", sorted(HYPER))
def test_one_step_per_element(name, t0):
    """p, exp_avg, exp_avg_sq and the EMA of one launch, element by element, within ``one_step_bounds`` of the float64
    step that uses the kernel's own bias corrections: the elementwise arithmetic alone.  The bounds are the derived ones,
    unwidened; measured on an MI355X the largest error / bound over all cases of this file is p 0.60, exp_avg 0.58,
    exp_avg_sq 0.49, EMA 0.22 (each case prints its own)."""
    rc, slabs, x, st = _one_step_run(name, t0)
    assert rc == 0
    hp = HYPER[name]
    _check_one_step(slabs, x, st, hp, LR, hp["wd"], GS_ONE_STEP[name] or 1.0, f"{name} t0={t0}")
    assert all(slabs[k].guards_intact() for k in "pmve") and slabs["g"].untouched()


@gpu
@pytest.mark.parametrize("t0", T0S)
@pytest.mark.parametrize("name", sorted(HYPER))
def test_tick_counter_and_bias_corrections(name, t0):
    """state[0] advances by exactly one; state[1], state[2] are within 2^-21 (four ulp of a value below 1) of
    1 - beta^t in double; the learning-rate slot is left alone"""
    rc, _, _, st = _one_step_run(name, t0)
    hp, t = HYPER[name], t0 + 1
    assert rc == 0 and st[0] == t and st[3] == np.float32(LR)
    for slot, b in ((1, hp["b1"]), (2, hp["b2"])):
        assert abs(float(st[slot]) - (1.0 - b ** t)) <= 2.0 ** -21, (slot, t, float(st[slot]), 1.0 - b ** t)


def _tiny_optimizer(name, lr=LR):
    from vmambair_amd.optim import FusedAdamEMA
    hp = HYPER[name]
    return FusedAdamEMA([torch.zeros(3, device=DEV)], None, lr=lr, betas=(0.9, 0.99 if name == "srgan" else 0.999),
                        eps=1e-8, weight_decay=hp["wd"])


@gpu
@pytest.mark.parametrize("t0", T0S)
@pytest.mark.parametrize("name", sorted(HYPER))
def test_loaded_bias_corrections_vs_tick(name, t0):
    """``load_state_dict`` at step t writes the corrections the tick kernel computes at the same t (to 2^-21, and both
    next to the double value), with the betas given as the Python doubles a user passes"""
    rc, _, _, st = _one_step_run(name, t0)
    hp, t = HYPER[name], t0 + 1
    fo = _tiny_optimizer(name)
    zero = torch.zeros(3, device=DEV)
    sd = fo.state_dict()
    sd["state"] = {0: {"step": torch.tensor(float(t)), "exp_avg": zero, "exp_avg_sq": zero}}
    fo.load_state_dict(sd)
    got = fo.state.cpu().numpy()
    assert rc == 0 and got[0] == t and got[3] == np.float32(LR)
    for slot, b in ((1, hp["b1"]), (2, hp["b2"])):
        assert abs(float(got[slot]) - float(st[slot])) <= 2.0 ** -21, (slot, t, float(got[slot]), float(st[slot]))
        assert abs(float(got[slot]) - (1.0 - b ** t)) <= 2.0 ** -21, (slot, t, float(got[slot]))


# offsets in floats past a 16-byte boundary of (param, grad, exp_avg, exp_avg_sq, ema); None = NULL
LAYOUTS = {"aligned": (0, 0, 0, 0, 0), "grad+1": (0, 1, 0, 0, 0), "grad+2": (0, 2, 0, 0, 0), "grad+3": (0, 3, 0, 0, 0),
           "param+1": (1, 0, 0, 0, 0), "ema+2": (0, 0, 0, 0, 2), "all_off": (1, 2, 3, 5, 6), "no_ema": (0, 0, 0, 0, None)}
LENGTHS = (1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 2047, 2048)


@gpu
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_chunk_lengths_and_pointer_alignment(layout, n):
    """One chunk of n elements (up to two trips of the 1024-element loop, ``valid < 4`` tails in either) under every
    pointer layout: the 16-byte path needs all five pointers aligned, everything else takes the per-element path, which
    is what the captured training step runs (gradient views into the flat buffer).  Results within the one-step bounds,
    every sentinel around p / exp_avg / exp_avg_sq / ema intact, the whole gradient buffer bit-unchanged although a clip
    coefficient of 0.25 is in use."""
    hp, s = HYPER["deraining"], 0.25
    x = _problem(n, 2, hp, 1000 + n, s)
    slabs, state = _slabs(x, LAYOUTS[layout]), _state(2)
    aligned = [slabs[k].ptr() % 16 == 0 for k in "pgmve" if slabs[k] is not None]
    assert all(aligned) == (layout in ("aligned", "no_ema"))
    scale = torch.tensor([s], dtype=torch.float32, device=DEV)
    assert _launch(slabs, state, hp, scale=scale) == 0
    _check_one_step(slabs, x, state.cpu().numpy(), hp, LR, hp["wd"], s, f"{layout} n={n}")
    for k in "pmve":
        assert slabs[k] is None or slabs[k].guards_intact(), f"{k}: written outside the chunk"
    assert slabs["g"].untouched(), "the gradient buffer was written"
    assert float(scale) == s


def _results(slabs):
    return [slabs[k].buf.clone() for k in "pmve"]


@gpu
def test_adam_entry_point_is_adamw_without_decay():
    """``oss_adam_ema_step`` = ``oss_adamw_ema_step`` with weight_decay = 0 and grad_scale = NULL, bit for bit"""
    # the identity: both run oss_adam_ema_kernel, and decay_keep = 1 - lr * 0 = 1 and gs = 1 multiply exactly
    hp = HYPER["srgan"]
    x = _problem(2500, 3, hp, 7, 1.0)
    out = []
    for entry in ("adam", "adamw"):
        slabs, state = _slabs(x, (0, 1, 0, 0, 0)), _state(3)
        assert _launch(slabs, state, hp, entry=entry, wd=0.0) == 0
        out.append(_results(slabs) + [state.clone()])
    assert all(torch.equal(a, b) for a, b in zip(*out))
    assert not torch.equal(out[0][0], _slabs(x, (0, 1, 0, 0, 0))["p"].buf), "the step changed nothing"


@gpu
def test_baked_lr_ignores_state_slot():
    """lr >= 0: the rate of the call is used and state[3] (here NaN) is never read; same bits as lr = -1 with the rate
    in state[3]"""
    hp = HYPER["deraining"]
    x = _problem(2500, 3, hp, 8, 1.0)
    out = []
    for lr_arg, slot in ((LR, float("nan")), (-1.0, LR)):
        slabs, state = _slabs(x), _state(3, slot)
        assert _launch(slabs, state, hp, lr_arg=lr_arg) == 0
        out.append(_results(slabs))
        st = state.cpu().numpy()
        assert st[0] == 4 and (np.isnan(st[3]) if lr_arg >= 0 else st[3] == np.float32(LR))
    assert all(torch.isfinite(a).all() for a in out[0])
    assert all(torch.equal(a, b) for a, b in zip(*out))


@gpu
@pytest.mark.parametrize("wd,s", [(f32(1e-2), None), (0.0, f32(0.3)), (f32(1e-2), f32(0.3))], ids=["decay", "scale", "both"])
def test_weight_decay_and_grad_scale_follow_float64(wd, s):
    """weight_decay = 1e-2 and a grad_scale < 1 each move the result where the float64 step says (one-step bounds), and
    away from the plain Adam result"""
    hp = HYPER["deraining"]
    x = _problem(2500, 3, hp, 9, s or 1.0)
    slabs, state = _slabs(x, (0, 3, 0, 0, 0)), _state(3)
    scale = None if s is None else torch.tensor([s], dtype=torch.float32, device=DEV)
    assert _launch(slabs, state, hp, wd=wd, scale=scale) == 0
    st = state.cpu().numpy()
    _check_one_step(slabs, x, st, hp, LR, wd, s or 1.0, f"wd={wd} s={s}")
    plain = ref_step(*(x[k].astype(np.float64) for k in "pmveg"), None, LR, hp["b1"], hp["b2"], hp["eps"], 0.0, hp["ema_decay"],
                     1.0, bc1=float(st[1]), bc2=float(st[2]))
    lim = one_step_bounds(x, plain, hp, LR, 0.0, 1.0)
    # (Adam's update hardly depends on the gradient's scale, so the scale shows in exp_avg; the decay shows in p)
    moved = (np.abs(slabs["p"].get() - plain[0]) > 4 * lim["p"]) | (np.abs(slabs["m"].get() - plain[1]) > 4 * lim["m"])
    assert moved.mean() > 0.5, "most elements must differ from the step without decay / scale"
    assert slabs["g"].untouched()


@gpu
def test_argument_errors_launch_nothing():
    """NULL table or NULL state: OSS_ERR_NULL; n_chunks = 0 or weight_decay = -1: OSS_ERR_SHAPE; nothing is launched"""
    code = {text.split(":")[0]: rc for rc, text in _capi.ERRORS.items()}
    hp = HYPER["deraining"]
    x = _problem(100, 3, hp, 10, 1.0)
    slabs, state = _slabs(x), _state(3)
    before = state.clone()
    for entry in ("adam", "adamw"):
        assert _launch(slabs, state, hp, entry=entry, table=None) == code["OSS_ERR_NULL"]
        assert _launch(slabs, state, hp, entry=entry, null_state=True) == code["OSS_ERR_NULL"]
        assert _launch(slabs, state, hp, entry=entry, n_chunks=0) == code["OSS_ERR_SHAPE"]
    assert _launch(slabs, state, hp, wd=-1.0) == code["OSS_ERR_SHAPE"]
    assert torch.equal(state[0], before[0]) and torch.equal(state[3], before[3]) and bool(torch.isnan(state[1:3]).all())
    assert all(slabs[k].untouched() for k in "pgmve")


@gpu
def test_zero_gradient_zero_moments():
    """g = 0, m = v = 0: the Adam term is 0 / eps = 0, so p' is fl(p * fl(1 - lr wd)) bit for bit and the moments stay 0;
    the EMA moves by its formula"""
    hp, wd = HYPER["deraining"], f32(1e-2)
    n = 1027
    x = _problem(n, 0, hp, 12, 1.0)
    x["g"] = np.zeros(n, np.float32)
    slabs, state = _slabs(x, (0, 1, 0, 0, 0)), _state(0)
    assert _launch(slabs, state, hp, wd=wd) == 0
    keep = np.float32(1.0) - np.float32(LR) * np.float32(wd)      # fp32 throughout
    assert keep == np.float32(1.0 - LR * wd), "contracted or not, 1 - lr wd rounds to the same float here"
    want_p = x["p"] * keep
    assert want_p.dtype == np.float32 and np.array_equal(slabs["p"].view.cpu().numpy(), want_p)
    assert not slabs["m"].get().any() and not slabs["v"].get().any()
    d = hp["ema_decay"]
    want_e = d * x["e"].astype(np.float64) + (1.0 - d) * want_p.astype(np.float64)
    assert (np.abs(slabs["e"].get() - want_e) <= 2.0 ** -22 * (np.abs(x["e"]) + np.abs(want_p))).all()
    assert not np.array_equal(slabs["e"].get(), x["e"].astype(np.float64))


# ---- FusedAdamEMA, as the training loop uses it ------------------------------------------------------------------------

NUMELS = (1, 5, 0, 21, 2049, 4096, 4097, 6145)     # one empty tensor: no chunk, and nothing breaks
SPANS = [(int(a), int(a + n)) for a, n in zip(np.cumsum((0,) + NUMELS[:-1]), NUMELS)]
TOTAL = sum(NUMELS)
CLIP = f32(0.01)


class Run:
    """parameters of NUMELS elements, their gradients in a real ``ddp.FlatGrads`` (unpadded, hence misaligned views)"""

    def __init__(self, p0, name, lr=LR, with_ema=True):
        from vmambair_amd.optim import FusedAdamEMA
        self.params = [torch.from_numpy(p0[a:b].copy()).to(DEV) for a, b in SPANS]
        self.ema = [p.clone() for p in self.params] if with_ema else None
        self.fo = FusedAdamEMA(self.params, self.ema, lr=lr, betas=(0.9, 0.99 if name == "srgan" else 0.999), eps=1e-8,
                               ema_decay=0.999, weight_decay=1e-4 if name == "deraining" else 0.0,
                               clip_grad_norm=0.01 if name == "deraining" else None)
        self.fg = None

    def load_grads(self, g):
        from vmambair_amd import ddp
        for p, (a, b) in zip(self.params, SPANS):
            p.grad = torch.from_numpy(g[a:b].copy()).to(DEV)
        if self.fg is None:
            self.fg = ddp.FlatGrads(self.params)
        self.fg.pack()
        assert all(p.grad.data_ptr() == v.data_ptr() for p, v in zip(self.params, self.fg.views))

    def step(self, g):
        self.load_grads(g)
        self.fo.step()

    @staticmethod
    def flat(tensors):
        return torch.cat([t.flatten() for t in tensors])

    def quantities(self):
        q = dict(p=self.flat(self.params), m=self.flat(self.fo.exp_avg), v=self.flat(self.fo.exp_avg_sq))
        if self.ema is not None:
            q["e"] = self.flat(self.ema)
        return q


def _trajectory_inputs(name, steps=64):
    rng = np.random.default_rng(5 if name == "srgan" else 6)
    p0 = rng.standard_normal(TOTAL).astype(np.float32)
    scale = 10.0 ** rng.uniform(-1.0, 1.0, steps)
    if name == "deraining":
        # the total norm is ~sqrt(TOTAL) = 128 times the scale: far above the clip norm of 0.01 on most steps, below it on three
        scale[[i for i in (3, 30, 50) if i < steps]] = 2e-5
    g = (rng.standard_normal((steps, TOTAL)) * scale[:, None]).astype(np.float32)
    return p0, g


def _torch_fp32_trajectory(name, p0, grads, lrs):
    """torch.optim.Adam / AdamW in fp32 on the CPU (foreach=False) after ``clip_grad_norm_``, and the EMA as the reference
    training writes it: an independent fp32 implementation whose distance from the float64 step sets the tolerance"""
    hp = HYPER[name]
    q = torch.from_numpy(p0.copy())
    ema = q.clone()
    cls = torch.optim.AdamW if hp["adamw"] else torch.optim.Adam
    opt = cls([q], lr=lrs[0], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=hp["wd"], foreach=False)
    for g, lr in zip(grads, lrs):
        opt.param_groups[0]["lr"] = lr
        q.grad = torch.from_numpy(g.copy())
        if name == "deraining":
            torch.nn.utils.clip_grad_norm_([q], CLIP, foreach=False)
        opt.step()
        ema.mul_(hp["ema_decay"]).add_(q, alpha=1.0 - hp["ema_decay"])
    st = opt.state[q]
    return dict(p=q.numpy(), m=st["exp_avg"].numpy(), v=st["exp_avg_sq"].numpy(), e=ema.numpy())


@gpu
@pytest.mark.parametrize("name", sorted(HYPER))
def test_trajectory_64_steps_all_quantities(name):
    """64 steps of ``FusedAdamEMA`` at lr 2e-2 over misaligned gradient views: p, exp_avg, exp_avg_sq and the EMA against
    the float64 step with double bias corrections (and, for the Deraining step, the clip coefficient in float64 from the
    same gradients).  srgan: Adam + EMA, ``set_lr(1e-2)`` after step 32; deraining: AdamW, clip norm 0.01, active on most
    steps and inactive on three, no EMA.

    Tolerance per quantity: 4x the largest error of torch's fp32 Adam(W) on the CPU against the same float64 step,
    floored per element by the one-step bounds summed over the 64 steps.  p, exp_avg (absolute; it cancels) and the EMA
    are compared absolutely, exp_avg_sq relatively.

    Measured on an MI355X, largest kernel error / largest torch-fp32 error (both are printed): srgan p 1.05 (1.9e-6 vs
    1.8e-6), exp_avg 0.93, exp_avg_sq 0.69 (5.1e-7 vs 7.4e-7 relative), EMA 0.53; deraining p 0.69 (7.4e-6 vs 1.1e-5),
    exp_avg 0.94, exp_avg_sq 0.67."""
    hp = HYPER[name]
    p0, grads = _trajectory_inputs(name)
    lrs = [LR] * 64 if name == "deraining" else [LR] * 32 + [f32(1e-2)] * 32
    run = Run(p0, name, with_ema=name == "srgan")
    coefs = []
    for t, g in enumerate(grads):
        run.step(g)
        if name == "deraining":
            coefs.append(float(run.fo.grad_scale))
        elif t == 31:
            run.fo.set_lr(1e-2)
    assert any(p.grad.data_ptr() % 16 for p in run.params), "the flat gradient views must be misaligned, as in production"
    assert float(run.fo.state[0]) == 64
    got = {k: t.cpu().numpy().astype(np.float64) for k, t in run.quantities().items()}

    p, e = p0.astype(np.float64), p0.astype(np.float64)
    m, v = np.zeros(TOTAL), np.zeros(TOTAL)
    floor = dict(p=np.zeros(TOTAL), m=np.zeros(TOTAL), e=np.zeros(TOTAL))
    want_coefs = []
    for t, (g, lr) in enumerate(zip(grads, lrs), 1):
        g = g.astype(np.float64)
        s = min(1.0, CLIP / (np.sqrt(np.sum(g * g)) + 1e-6)) if name == "deraining" else 1.0
        want_coefs.append(s)
        x = dict(p=p, g=g, m=m, e=e)
        ref = ref_step(p, m, v, e, g, t, lr, hp["b1"], hp["b2"], hp["eps"], hp["wd"], hp["ema_decay"], s)
        lim = one_step_bounds(x, ref, hp, lr, hp["wd"], s)
        for k in floor:
            floor[k] += lim[k]
        p, m, v, e = ref
    want = dict(p=p, m=m, v=v, e=e)
    if name == "deraining":
        active = sum(c < 1.0 for c in coefs)
        assert active > 32 and 64 - active >= 1, coefs
        assert np.allclose(coefs, want_coefs, rtol=1e-5, atol=0)

    th = _torch_fp32_trajectory(name, p0, grads, lrs)
    gmax = float(max(np.abs(g).max() * s for g, s in zip(grads, want_coefs)))
    bad = {}
    for k in got:
        if k == "v":
            ek, et = np.abs(got[k] - want[k]) / want[k], np.abs(th[k] - want[k]) / want[k]
            fl = np.full(TOTAL, 64 * 2.0 ** -21)
        else:
            ek, et, fl = np.abs(got[k] - want[k]), np.abs(th[k] - want[k]), floor[k]
        tol = np.maximum(4.0 * et.max(), fl)
        unit = "relative" if k == "v" else "of max|g| %.3e" % gmax if k == "m" else "absolute"
        print(f"[trajectory {name}] {k}: kernel {ek.max():.3e}, torch fp32 {et.max():.3e}, ratio {ek.max() / et.max():.2f}; "
              f"floor {fl.min():.3e} .. {fl.max():.3e} ({unit}" + (f"; kernel {ek.max() / gmax:.3e}" if k == "m" else "") + ")")
        if (ek > tol).any():
            bad[k] = (float(ek.max()), float(et.max()))
    assert not bad, bad


@gpu
def test_resume_from_state_dict_continues_bitwise():
    """8 steps, ``state_dict()`` into a fresh ``FusedAdamEMA`` (built with another learning rate), 8 more steps: the same
    bits as 16 uninterrupted steps.  The loaded bias corrections play no part: the next tick recomputes them from t."""
    name = "deraining"
    p0, grads = _trajectory_inputs(name, steps=16)
    whole, first = Run(p0, name, with_ema=False), Run(p0, name, with_ema=False)
    for g in grads:
        whole.step(g)
    for g in grads[:8]:
        first.step(g)
    sd = first.fo.state_dict()
    assert float(sd["state"][0]["step"]) == 8 and len(sd["state"]) == len(NUMELS)
    second = Run(Run.flat(first.params).cpu().numpy(), name, lr=1.0, with_ema=False)
    second.fo.load_state_dict(sd)
    assert second.fo.lr == LR and float(second.fo.state[3]) == LR
    for g in grads[8:]:
        second.step(g)
    a, b = whole.quantities(), second.quantities()
    assert float(second.fo.state[0]) == 16
    for k in "pmv":
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["p"], Run.flat(first.params))


@gpu
def test_captured_replay_same_bits_as_eager():
    """one ``step()`` captured in a graph over the static flat gradient buffer and replayed 5 times with new gradient
    contents: the same bits as 5 eager steps of a twin; the step counter advances by one per replay"""
    name = "deraining"
    p0, grads = _trajectory_inputs(name, steps=6)
    cap, twin = Run(p0, name), Run(p0, name)
    cap.load_grads(grads[5])
    live = cap.params + cap.ema + cap.fo.exp_avg + cap.fo.exp_avg_sq + [cap.fo.state]
    snap = [t.clone() for t in live]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):              # lazy initialisation happens outside the capture, as in train_graph.py
        cap.fo.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t, s in zip(live, snap):
        t.copy_(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap.fo.step()
    assert float(cap.fo.state[0]) == 0, "capturing must not run the step"
    for k in range(5):
        cap.fg.flat.copy_(torch.from_numpy(grads[k]).to(DEV))
        graph.replay()
        twin.step(grads[k])
        assert float(cap.fo.state[0]) == k + 1 == float(twin.fo.state[0])
    a, b = cap.quantities(), twin.quantities()
    for k in "pmve":
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["p"], Run.flat(snap[:len(NUMELS)]))
