"""One decoder of ``oss_dtype`` (``io_dispatch``, csrc/oss_host.h): a value that is no element type is refused before anything runs.

One entry point per translation unit is called with ``io = 7`` (out of range) and -- the ones that are not GEMM-shaped, which do
not take the selector -- with ``OSS_F32_BF16X3``, on real device tensors of the smallest shape the kernel accepts.  Every buffer is
sized for 4-byte elements, so no decode of the value could leave it; the outputs are prefilled with a sentinel.  The call has to
return ``OSS_ERR_SHAPE`` and leave the sentinel intact (until this decoder, most launchers read every value they did not name as
bf16 and launched)."""
import ctypes as C

import pytest
import torch

from vmambair_amd import _capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_SHAPE = -2
SENTINEL = -12345.0
F32, X3, BAD = _capi.OSS_F32, _capi.OSS_F32_BF16X3, 7
B, CH, H, W = 1, 16, 8, 8            # the default shape
D, R, N, L = 96, 3, 16, 64           # the projection: C = R + 2 N rows of x_dbl
CP = R + 2 * N


def _in(*shape):
    g = torch.Generator().manual_seed(sum(shape))
    return torch.randn(*shape, generator=g).to(DEV)


def _out(*shape, dtype=torch.float32):
    return torch.full(shape, SENTINEL, dtype=dtype, device=DEV)


def _p(t):
    return None if t is None else t.data_ptr()


# each case: name -> f(lib, io, stream) -> (return code, output tensors).  `io` goes where the entry point takes its oss_dtype.
def _merge4(lib, io, st):
    out, y = _in(B, 4, CH, H * W), _out(B, CH, H, W)
    return lib.oss_merge4(io, _p(out), _p(y), B, CH, H, W, st), [y]


def _gelu_gate(lib, io, st):
    n = CH * H * W
    h, out = _in(B, 2, n), _out(B, n)
    return lib.oss_gelu_gate_fwd(io, _p(h), _p(out), B, n, 2 * n, st), [out]


def _cross_scan2_in(lib, io, st):
    x, x2 = _in(B, CH, H, W), _out(B, 2, CH, H * W)
    return lib.oss_cross_scan2(io, F32, _p(x), _p(x2), B, CH, H, W, CH * H * W, H * W, st), [x2]


def _cross_scan2_out(lib, io, st):
    x, x2 = _in(B, CH, H, W), _out(B, 2, CH, H * W)
    return lib.oss_cross_scan2(F32, io, _p(x), _p(x2), B, CH, H, W, CH * H * W, H * W, st), [x2]


def _dwconv(lib, io, st):
    x, w, b, y = _in(B, CH, H, W), _in(CH, 9), _in(CH), _out(B, CH, H, W)
    return lib.oss_dwconv3x3_fwd(io, _p(x), _p(w), _p(b), _p(y), None, B, CH, H, W, CH * H * W, H * W, CH * H * W, H * W, 0, st), [y]


def _dwgate(lib, io, st):
    hd, h, w_ = CH // 2, 64, 64       # the gate's kernels work on 64-pixel planes
    t, w, b, out = _in(B, 2 * hd, h, w_), _in(2 * hd, 9), _in(2 * hd), _out(B, hd, h, w_)
    return lib.oss_dwgate_fwd(io, _p(t), _p(w), _p(b), _p(out), B, hd, h, w_, 2 * hd * h * w_, h * w_, hd * h * w_, h * w_, st), [out]


def _conv3x3_thin(lib, io, st):
    cout = 3
    x, w, b, y = _in(B, CH, H, W), _in(cout, CH, 3, 3), _in(cout), _out(B, cout, H, W)
    return lib.oss_conv3x3_thin_fwd(io, _p(x), _p(w), _p(b), _p(y), B, CH, cout, H, W, CH * H * W, H * W, cout * H * W, H * W, st), [y]


def _conv3x3_dense(lib, io, st):
    x, w, b, y = _in(B, CH, H, W), _in(CH, CH, 3, 3), _in(CH), _out(B, CH, H, W)
    return lib.oss_conv3x3_dense_fwd(io, _p(x), _p(w), _p(b), _p(y), B, CH, CH, H, W, CH * H * W, H * W, CH * H * W, H * W, st), [y]


def _conv1x1(lib, io, st):
    x, w, b, y = _in(B, CH, H * W), _in(CH, CH), _in(CH), _out(B, CH, H * W)
    return lib.oss_conv1x1_fwd(io, _p(x), _p(w), _p(b), None, _p(y), B, CH, CH, H * W, CH * H * W, H * W, st), [y]


def _proj(lib, io, st):
    x2, wx, wdt = _in(B, 2, D, L), _in(4, CP, D), _in(4, D, R)
    xdbl, dts = _out(B, 4, CP, L), _out(B, 4, D, L)
    return lib.oss_proj_fwd(io, _p(x2), _p(wx), _p(wdt), _p(xdbl), _p(dts), B, D, CP, R, L, st), [xdbl, dts]


def _ln(lib, xt, yt, st):
    p = H * W
    x, w, b = _in(B, CH, p), _in(CH), _in(CH)
    y, mean, rstd = _out(B, CH, p), _out(B, p), _out(B, p)
    rc = lib.oss_ln_nchw_fwd(xt, yt, _p(x), _p(w), _p(b), None, _p(y), _p(mean), _p(rstd), B, CH, p, CH * p, p, 0, 0, 1e-5, st)
    return rc, [y, mean, rstd]


def _ln_x(lib, io, st):
    return _ln(lib, io, F32, st)


def _ln_y(lib, io, st):
    return _ln(lib, F32, io, st)


def _rowsum(lib, io, st):
    p = H * W
    a, out = _in(B, CH, p), _out(B, CH)
    return lib.oss_rowsum(io, _p(a), None, _p(out), B, CH, p, CH * p, p, 0, 0, 1.0, st), [out]


def _row_affine(lib, io, st):
    p = H * W
    x, mul, y = _in(B, CH, p), _in(B, CH), _out(B, CH, p)
    return lib.oss_row_affine(io, _p(x), _p(mul), None, _p(y), B, CH, p, CH * p, p, 1.0, st), [y]


def _image_metrics(lib, io, st):
    c, h, w = 3, 16, 16
    a, b = _in(B, c, h, w), _in(B, c, h, w)
    n = lib.oss_image_metrics_partial_doubles(B, c, h, w, 0)
    assert n > 0
    out, part = _out(B, 2, dtype=torch.float64), _out(n, dtype=torch.float64)
    rc = lib.oss_image_metrics(io, _p(a), _p(b), _p(out), _p(part), B, c, h, w, c * h * w, h * w, w, c * h * w, h * w, w, 0,
                               _capi.METRIC_REPLICATE, st)
    return rc, [out, part]


def _scan_fwd(lib, io, st):
    dim, n, seq, groups = CH, 16, 64, 1
    u, delta, a = _in(B, dim, seq), _in(B, dim, seq), -torch.rand(dim, n, device=DEV)
    bm, cm = _in(B, groups, n, seq), _in(B, groups, n, seq)
    out, x = _out(B, dim, seq), _out(B, dim, lib.oss_scan_num_chunks(seq), 2 * n)
    p = _capi.ScanFwdParams()
    p.batch, p.dim, p.seqlen, p.dstate, p.n_groups, p.delta_softplus, p.rev_group_start = B, dim, seq, n, groups, 1, groups
    p.u_batch_stride = p.delta_batch_stride = p.out_batch_stride = dim * seq
    p.u_d_stride = p.delta_d_stride = p.out_d_stride = seq
    p.A_d_stride = n
    p.B_batch_stride = p.C_batch_stride = groups * n * seq
    p.B_group_stride = p.C_group_stride = n * seq
    p.B_dstate_stride = p.C_dstate_stride = seq
    p.u, p.delta, p.B, p.C, p.out = _p(u), _p(delta), _p(bm), _p(cm), _p(out)
    p.A, p.x = _p(a), _p(x)
    return lib.oss_scan_fwd(C.byref(p), io, st), [out, x]


GEMM_SHAPED = {"oss_conv1x1_fwd": _conv1x1, "oss_proj_fwd": _proj}     # OSS_F32_BF16X3 is theirs to take
OTHERS = {"oss_merge4": _merge4, "oss_gelu_gate_fwd": _gelu_gate, "oss_cross_scan2[in]": _cross_scan2_in,
          "oss_cross_scan2[out]": _cross_scan2_out, "oss_dwconv3x3_fwd": _dwconv, "oss_dwgate_fwd": _dwgate,
          "oss_conv3x3_thin_fwd": _conv3x3_thin, "oss_conv3x3_dense_fwd": _conv3x3_dense, "oss_ln_nchw_fwd[x]": _ln_x,
          "oss_ln_nchw_fwd[y]": _ln_y, "oss_rowsum": _rowsum, "oss_row_affine": _row_affine, "oss_image_metrics": _image_metrics,
          "oss_scan_fwd": _scan_fwd}
CASES = [(name, BAD) for name in GEMM_SHAPED] + [(name, io) for name in OTHERS for io in (BAD, X3)]


@pytest.mark.parametrize("name,io", CASES, ids=[f"{n}-io{io}" for n, io in CASES])
def test_a_value_that_is_no_element_type_is_refused_before_anything_runs(name, io):
    lib = _capi.load()
    call = GEMM_SHAPED.get(name) or OTHERS[name]
    rc, outputs = call(lib, io, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == ERR_SHAPE, (name, io, rc)
    for t in outputs:
        assert bool((t == SENTINEL).all()), (name, io)


def test_the_same_calls_run_with_an_element_type():
    """the cases above are refused for their dtype, not for their shape: with OSS_F32 each call is taken and writes its output"""
    lib = _capi.load()
    st = torch.cuda.current_stream().cuda_stream
    for name, call in {**GEMM_SHAPED, **OTHERS}.items():
        if name in ("oss_conv3x3_thin_fwd", "oss_conv3x3_dense_fwd"):
            continue   # 16-bit kernels only: OSS_F32 is refused by design (tests/test_conv3x3_gpu.py runs them)
        rc, outputs = call(lib, F32, st)
        torch.cuda.synchronize()
        assert rc == 0, (name, rc)
        assert not bool((outputs[0] == SENTINEL).any()), name
