"""The channel-branch kernels evaluate the lift and the two projections as affine functions of the pooled scalar inside the scan
lanes (oss_channel.hip).  ``ChannelGateFn`` is called directly with hand-built parameters, so the scan length L = d_inner is free:
a single step, one lane, both sides of a 128-step chunk boundary, an odd tail, three chunks.  The reference is the literal dense
data flow in float64 (lift, two einsums, a sequential scan loop, conv_cout, layer_norm, gate) with autograd.  A CPU-only test checks
the algebra itself in float64."""
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close

DEV = "cuda:0"
N = 16
NAMES = ["cin_w", "cin_b", "Wxc", "Wdtc", "dt_bias", "A_logs", "Dsc", "cout_w", "cout_b", "cn_w", "cn_b"]
CFGS = {"dc1_r3": (1, 3, False), "dc2_r6": (2, 6, True), "dc4_r6": (4, 6, True)}   # dc, Rc, lift


def _params(L, dc, Rc, lift, seed):
    """float64 parameters with the scales of SS2D_1's initialisation; Ac_logs and dtc_projs_bias halved so the scan does not saturate"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    un = lambda bound, *s: (torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) * bound
    p = dict(cin_w=un(1.0, dc, 1, 1, 1) if lift else None, cin_b=un(1.0, dc) if lift else None,
             Wxc=un(dc ** -0.5, 2, Rc + 2 * N, dc), Wdtc=rn(2, dc, Rc), dt_bias=0.5 * rn(2, dc), A_logs=0.5 * rn(2 * dc, N),
             Dsc=1.0 + 0.1 * rn(2 * dc), cout_w=un(dc ** -0.5, 1, dc, 1, 1) if lift else None, cout_b=un(dc ** -0.5, 1) if lift else None,
             cn_w=1.0 + 0.1 * rn(L), cn_b=0.1 * rn(L))
    return p


def _dense_projections(pooled, cin_w, cin_b, Wxc, Wdtc):
    """pooled (b, L) -> xsc (b, 2, dc, L), z (b, 2, Cc, L), dts (b, 2, dc, L): direction 1 walks the channels backwards"""
    seq = pooled[:, None, :] if cin_w is None else pooled[:, None, :] * cin_w.view(1, -1, 1) + cin_b.view(1, -1, 1)
    xsc = torch.stack([seq, seq.flip(-1)], dim=1)
    z = torch.einsum("bkdl,kcd->bkcl", xsc, Wxc)
    dts = torch.einsum("bkrl,kdr->bkdl", z[:, :, :Wdtc.shape[2]], Wdtc)
    return xsc, z, dts


def _reference(y2, p, mul_mode):
    b, d = y2.shape[:2]
    Rc, dc = p["Wdtc"].shape[2], p["Wdtc"].shape[1]
    xsc, z, dts = _dense_projections(y2.mean(dim=(2, 3)), p["cin_w"], p["cin_b"], p["Wxc"], p["Wdtc"])
    Bs, Cs = z[:, :, Rc:Rc + N], z[:, :, Rc + N:]
    delta = F.softplus(dts + p["dt_bias"].view(1, 2, dc, 1), threshold=20.0)
    A = -torch.exp(p["A_logs"]).view(1, 2, dc, N)
    h = torch.zeros(b, 2, dc, N, dtype=y2.dtype)
    ys = []
    for l in range(d):
        dl = delta[..., l, None]
        h = torch.exp(dl * A) * h + dl * Bs[:, :, None, :, l] * xsc[..., l, None]
        ys.append((h * Cs[:, :, None, :, l]).sum(-1))
    y = torch.stack(ys, dim=-1) + p["Dsc"].view(1, 2, dc, 1) * xsc
    y = y[:, 0] + y[:, 1].flip(-1)
    yc = y.reshape(b, d) if p["cout_w"] is None else (y * p["cout_w"].view(1, dc, 1)).sum(1) + p["cout_b"]
    c = F.layer_norm(yc, (d,), p["cn_w"], p["cn_b"], 1e-5)[:, :, None, None]
    return y2 * c + y2 if mul_mode else y2 + c


@functools.lru_cache(maxsize=None)
def _case(L, cfg, mul_mode):
    """inputs and the float64 reference of one case, computed once"""
    dc, Rc, lift = CFGS[cfg]
    p = _params(L, dc, Rc, lift, seed=1000 * L + dc)
    g = torch.Generator().manual_seed(7 * L + dc)
    y2 = torch.randn(2, L, 4, 4, generator=g, dtype=torch.float64)
    gout = torch.randn(2, L, 4, 4, generator=g, dtype=torch.float64)
    leaves = {k: v.clone().requires_grad_() for k, v in p.items() if v is not None}
    yi = y2.clone().requires_grad_()
    out = _reference(yi, {k: leaves.get(k) for k in NAMES}, mul_mode)
    out.backward(gout)
    return p, y2, gout, out.detach(), yi.grad, {k: v.grad for k, v in leaves.items()}


def _gpu_run(p, y2, gout, mul_mode):
    from vmambair_amd import ops
    prm = [None if p[k] is None else p[k].float().to(DEV).requires_grad_() for k in NAMES]
    yi = y2.float().to(DEV).requires_grad_()
    out = ops.ChannelGateFn.apply(yi, *prm, mul_mode)
    out.backward(gout.float().to(DEV))
    return out.detach(), yi.grad, {k: t.grad for k, t in zip(NAMES, prm) if t is not None}


@pytest.mark.gpu
@pytest.mark.parametrize("mul_mode", [True, False], ids=["mul_add", "add"])
@pytest.mark.parametrize("cfg", list(CFGS))
@pytest.mark.parametrize("L", [1, 2, 127, 128, 129, 257])
def test_channel_gate_against_the_dense_float64_data_flow(L, cfg, mul_mode):
    p, y2, gout, out_r, dy_r, g_r = _case(L, cfg, mul_mode)
    out, dy, gr = _gpu_run(p, y2, gout, mul_mode)
    out2, dy2, gr2 = _gpu_run(p, y2, gout, mul_mode)
    assert torch.equal(out, out2) and torch.equal(dy, dy2), "a second run of the same call differs"
    assert set(gr) == set(gr2) == set(g_r)
    for k in gr:
        assert torch.equal(gr[k], gr2[k]), f"a second run of the same call differs: {k}"
    assert_close(out, out_r, 2e-4, 2e-4 * float(out_r.abs().max()), "out")
    assert_close(dy, dy_r, 2e-3, 5e-4 * float(dy_r.abs().max()), "dy2")
    for k in g_r:
        if k == "cout_b":
            continue  # exact gradient 0 (a constant in front of a LayerNorm)
        assert gr[k].shape == g_r[k].shape, k
        assert_close(gr[k], g_r[k], 5e-3, 1e-3 * max(float(g_r[k].abs().max()), 1e-6), k)


@pytest.mark.parametrize("cfg", list(CFGS))
def test_coefficient_form_is_the_dense_form_in_float64(cfg):
    """No GPU.  z and dts of the dense data flow against  za p + zb  and  ta p + tb; then, for arbitrary cotangents of the B / C
    columns of z, of dts and of u, the kernels' map from the coefficient gradients to d pooled and to the gradients of xc_proj,
    dtc_projs, conv_cin against autograd of the dense form.  1e-12 relative: a sign or index slip is O(1)."""
    dc, Rc, lift = CFGS[cfg]
    L, b = 37, 1
    p = _params(L, dc, Rc, lift, seed=5)
    g = torch.Generator().manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    pooled = rn(b, L).requires_grad_()
    leaves = {k: p[k].clone().requires_grad_() for k in ("cin_w", "cin_b", "Wxc", "Wdtc") if p[k] is not None}
    xsc, z, dts = _dense_projections(pooled, leaves.get("cin_w"), leaves.get("cin_b"), leaves["Wxc"], leaves["Wdtc"])
    Gz, Gd, Gu = rn(*z.shape), rn(*dts.shape), rn(*xsc.shape)
    Gz[:, :, :Rc] = 0   # the dt columns of z feed dts only

    def close(a, want, what):
        err = float((a - want).abs().max()) / max(float(want.abs().max()), 1e-300)
        assert err <= 1e-12, f"{what}: relative error {err:.3e}"

    # coefficient table
    cw = p["cin_w"].view(dc) if lift else torch.ones(dc, dtype=torch.float64)
    cb = p["cin_b"] if lift else torch.zeros(dc, dtype=torch.float64)
    Wxc, Wdtc = p["Wxc"], p["Wdtc"]
    za, zb = Wxc @ cw, Wxc @ cb                                                    # (2, Cc)
    ta, tb = torch.einsum("kir,kr->ki", Wdtc, za[:, :Rc]), torch.einsum("kir,kr->ki", Wdtc, zb[:, :Rc])
    pk = torch.stack([pooled.detach(), pooled.detach().flip(-1)], dim=1)           # (b, 2, L): p at the step of each direction
    close(za[None, :, :, None] * pk[:, :, None, :] + zb[None, :, :, None], z.detach(), "z")
    close(ta[None, :, :, None] * pk[:, :, None, :] + tb[None, :, :, None], dts.detach(), "dts")
    close(cw[None, None, :, None] * pk[:, :, None, :] + cb[None, None, :, None], xsc.detach(), "u")

    # dense gradients by autograd
    ((z * Gz).sum() + (dts * Gd).sum() + (xsc * Gu).sum()).backward()

    # the kernels' form: sums over the steps weighted with p and plain, then the small map
    dza, dzb = (Gz * pk[:, :, None, :]).sum(dim=(0, 3)), Gz.sum(dim=(0, 3))         # (2, Cc); dt columns still 0
    dta, dtb = (Gd * pk[:, :, None, :]).sum(dim=(0, 3)), Gd.sum(dim=(0, 3))         # (2, dc)
    dcw, dcb = (Gu * pk[:, :, None, :]).sum(dim=(0, 1, 3)), Gu.sum(dim=(0, 1, 3))   # (dc)
    dza[:, :Rc] = torch.einsum("kir,ki->kr", Wdtc, dta)
    dzb[:, :Rc] = torch.einsum("kir,ki->kr", Wdtc, dtb)
    close(dta[:, :, None] * za[:, None, :Rc] + dtb[:, :, None] * zb[:, None, :Rc], leaves["Wdtc"].grad, "d dtc_projs_weight")
    close(dza[:, :, None] * cw + dzb[:, :, None] * cb, leaves["Wxc"].grad, "d xc_proj_weight")
    if lift:
        close(dcw + torch.einsum("kci,kc->i", Wxc, dza), leaves["cin_w"].grad.view(dc), "d conv_cin.weight")
        close(dcb + torch.einsum("kci,kc->i", Wxc, dzb), leaves["cin_b"].grad, "d conv_cin.bias")
    # d pooled: per step  sum_c za dz + sum_i (ta g_delta + cw du), direction 1 un-flipped
    dpk = (za[None, :, Rc:, None] * Gz[:, :, Rc:]).sum(2) + (ta[None, :, :, None] * Gd).sum(2) + (cw[None, None, :, None] * Gu).sum(2)
    close(dpk[:, 0] + dpk[:, 1].flip(-1), pooled.grad, "d pooled")
