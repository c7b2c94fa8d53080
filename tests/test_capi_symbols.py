"""The C-ABI library: loads without a GPU, exports every symbol include/vmambair_oss.h declares, and the ctypes binding that
vmambair_amd/_cheader.py reads out of that header has the prototypes and the struct layout a C compiler gives them.  No compute
calls here."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import vmambair_amd
from vmambair_amd import _build, _capi, _cheader

HEADER = _build.HEADER


def _stripped_header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _declared_functions():
    return sorted(set(re.findall(r"\b(oss_[a-z_0-9]+)\s*\(", _stripped_header())))


def test_library_is_built_and_loads():
    assert os.path.exists(_build.LIB_PATH), "run __graft_entry__.build() first"
    lib = _capi.load()
    assert lib.oss_version().startswith(b"vmambair_oss")
    assert lib.oss_scan_chunk() == 256
    assert lib.oss_scan_num_chunks(1) == 1 and lib.oss_scan_num_chunks(256) == 1
    assert lib.oss_scan_num_chunks(257) == 2 and lib.oss_scan_num_chunks(4096) == 16


def test_every_declared_symbol_is_exported():
    declared = _declared_functions()
    assert declared == sorted(_capi.SYMBOLS)
    assert declared == sorted(_cheader.read(HEADER).prototypes), "the header reader dropped or invented a prototype"
    lib = ctypes.CDLL(_build.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in the header but not exported"


def test_prototypes_are_complete():
    """after load() every declared function carries a full prototype; the parameter count comes from a plain comma count of the
    header's text, not from the reader"""
    lib = _capi.load()
    found = re.findall(r"\b(oss_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", _stripped_header())
    assert sorted(n for n, _ in found) == _declared_functions()
    for name, args in found:
        fn = getattr(lib, name)
        n_params = 0 if args.strip() == "void" else args.count(",") + 1
        assert fn.argtypes is not None and len(fn.argtypes) == n_params, name
        assert fn.restype in (ctypes.c_int, ctypes.c_size_t, ctypes.c_char_p, None), name


def test_struct_layout_matches_header():
    """Compile a C probe against the header that prints sizeof and every field's offsetof of all seven structs, generated from
    the parsed field lists, and compare with the ctypes classes."""
    structs = _cheader.read(HEADER).structs
    assert list(structs) == ["oss_scan_fwd_params", "oss_scan_bwd_params", "oss_scan_launch", "oss_conv1x1_launch", "oss_chan_params", "oss_sum_chunk", "oss_adam_chunk"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vmambair_oss.h"', 'int main(void) {']
    want = []
    for name, cls in structs.items():
        lines.append(f'  printf("%zu\\n", sizeof({name}));')
        want.append(ctypes.sizeof(cls))
        for field, _ in cls._fields_:
            lines.append(f'  printf("%zu\\n", offsetof({name}, {field}));')
            want.append(getattr(cls, field).offset)
    lines.append('  return 0; }')
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "probe.c")
        open(c, "w").write("\n".join(lines))
        exe = os.path.join(td, "probe")
        subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert len(want) > 100 and got == want
    # the classes the package hands out are that layout
    for name, cls in (("oss_scan_fwd_params", _capi.ScanFwdParams), ("oss_scan_bwd_params", _capi.ScanBwdParams),
                      ("oss_chan_params", _capi.ChanParams), ("oss_adam_chunk", _capi.AdamChunk)):
        assert [(f, getattr(cls, f).offset) for f, _ in cls._fields_] == [(f, getattr(structs[name], f).offset) for f, _ in structs[name]._fields_]
        assert ctypes.sizeof(cls) == ctypes.sizeof(structs[name])
    assert _capi.SUM_CHUNK_BYTES == ctypes.sizeof(structs["oss_sum_chunk"]) == 40
    assert _capi.ScanBwdParams.f.offset == 0 and _capi.ScanBwdParams._fields_[0][1] is _capi.ScanFwdParams


def test_every_error_code_has_a_message():
    constants = _cheader.read(HEADER).constants
    codes = {n: v for n, v in constants.items() if n.startswith("OSS_ERR_")}
    assert len(codes) >= 4 and constants["OSS_OK"] == 0
    for name, value in codes.items():
        assert value < 0 and _capi.ERRORS[value].startswith(name + ":"), name
    assert _capi.ABI_VERSION == constants["OSS_ABI_VERSION"] and _capi.ADAM_CHUNK == constants["OSS_ADAM_CHUNK"] == 2048
    assert (_capi.OSS_F32, _capi.OSS_F16, _capi.OSS_BF16, _capi.OSS_F32_BF16X3) == (0, 1, 2, 3)
    assert (_capi.METRIC_QUANTISE, _capi.METRIC_Y, _capi.METRIC_REPLICATE) == (1, 2, 4)
    assert (_capi.FEATURE_FUSED_DT, _capi.FEATURE_LANE_STATES) == (1, 2)


_SNIPPET = """
/* a header in the subset */
#ifndef GUARD_H
#define GUARD_H
#include <stdint.h>
extern "C" {
#define X (-4)
#define OSS_Y 7     /* trailing comment */
typedef enum { OSS_A = 0, OSS_B = 5 } oss_dtype;
typedef void *oss_stream_t;
typedef struct {
    int n, m;
    const float *a, *b;   /* the star belongs to the declarator */
    int64_t stride;
    float scale;
} oss_inner_params;
typedef struct {
    oss_inner_params f;
    void *out;
    size_t bytes;
} oss_outer_params;
typedef struct { void *p; int n, reserved_; } oss_row;
int oss_last(int which /* 0 fwd, 1 bwd */);
const char *oss_version(void);
void oss_reset(void);
size_t oss_wrapped(oss_dtype io, const oss_outer_params *p,
                   int64_t stride, const oss_row *rows,
                   float eps, oss_stream_t stream);
int oss_names(int i, const char **name, double *sum, long long *calls, double x, long long);
}
#endif
"""


def test_reader_on_synthetic_snippets():
    C = ctypes
    h = _cheader.parse(_SNIPPET)
    assert h.constants == {"X": -4, "OSS_Y": 7, "OSS_A": 0, "OSS_B": 5}
    inner, outer, row = (h.structs[n] for n in ("oss_inner_params", "oss_outer_params", "oss_row"))
    assert list(h.structs) == ["oss_inner_params", "oss_outer_params", "oss_row"]
    assert inner._fields_ == [("n", C.c_int), ("m", C.c_int), ("a", C.c_void_p), ("b", C.c_void_p), ("stride", C.c_int64),
                              ("scale", C.c_float)]
    assert outer._fields_ == [("f", inner), ("out", C.c_void_p), ("bytes", C.c_size_t)]
    assert C.sizeof(inner) == 40 and outer.out.offset == 40 and C.sizeof(outer) == 56 and C.sizeof(row) == 16
    assert h.prototypes == {
        "oss_last": (C.c_int, [C.c_int]),
        "oss_version": (C.c_char_p, []),
        "oss_reset": (None, []),
        "oss_wrapped": (C.c_size_t, [C.c_int, C.POINTER(outer), C.c_int64, C.c_void_p, C.c_float, C.c_void_p]),
        "oss_names": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_longlong]),
    }
    assert list(h.prototypes) == ["oss_last", "oss_version", "oss_reset", "oss_wrapped", "oss_names"]


@pytest.mark.parametrize("bad, names", [
    ("int oss_f(unsigned short x);", "unsigned short"),                         # a type outside the table
    ("typedef struct { unsigned short x; } oss_s;", "unsigned short"),
    ("int oss_f(int n, void (*callback)(int));", "callback"),                   # function pointer
    ("int oss_f(int n);\nsize_t oss_g(void);\nint oss_f(int n);", "oss_f"),     # duplicate prototype
    ("#define OSS_A 1\ntypedef enum { OSS_A = 1 } oss_e;", "OSS_A"),            # duplicate constant
    ("typedef struct { int a[4]; } oss_s;", "a[4]"),                            # array field
    ("typedef union { int a; float b; } oss_u;", "union"),                      # a typedef it cannot read
    ("int oss_f(int n, ...);", "..."),
    ("int oss_f(int n)", "oss_f"),                                              # no terminating semicolon
    ("#define OSS_A (1 << 3)", "1 << 3"),
    ("static int oss_f(int n);", "static"),
])
def test_reader_refuses_what_it_cannot_read(bad, names):
    with pytest.raises(RuntimeError) as e:
        _cheader.parse(bad)
    assert names in str(e.value)


def test_workspace_query_is_pure():
    lib = _capi.load()
    n = lib.oss_scan_bwd_workspace_bytes(2, 8, 100, 16, 4)
    tiles = (2 + 3) // 4  # 2 rows per group, 4 rows per workgroup in the smallest variant (bwd variant 1)
    # per row tile: dB / dC partial rows (2 * dstate) + 8 rows for the fused-delta form; per (batch, row): dA, dD, dbias, 8 dt weights
    assert n == 4 * (2 * 4 * tiles * (2 * 16 + 8) * 100 + 2 * 8 * (18 + 8))
    assert lib.oss_scan_bwd_workspace_bytes(2, 7, 100, 16, 4) == 0  # dim % n_groups != 0
    # long sequences: room for time-segmented launches -- one weight-gradient partial per (batch, segment, row) and the
    # reverse-carry pairs; segments are counted in 512-step chunks, at most 64
    n = lib.oss_scan_bwd_workspace_bytes(1, 8, 2048, 16, 4)
    assert n == 4 * (1 * 4 * 1 * (2 * 16 + 8) * 2048 + 1 * 4 * 8 * (18 + 8) + 2 * 1 * 8 * 16 * 4)
    # forward: (prod a, h) per (batch, row, segment, state); segments counted in 256-step chunks, at most 64; none needed below
    assert lib.oss_scan_fwd_workspace_bytes(2, 8, 256, 16, 4) == 0
    assert lib.oss_scan_fwd_workspace_bytes(2, 8, 1000, 16, 4) == 4 * 2 * 2 * 8 * 16 * 4
    assert lib.oss_scan_fwd_workspace_bytes(1, 384, 160 * 160, 16, 4) == 4 * 2 * 384 * 16 * 64


def test_segment_override_round_trips_without_a_gpu():
    lib = _capi.load()
    lib.oss_scan_set_segments(3, 5)
    lib.oss_scan_set_segments(-1, -1)
    assert lib.oss_scan_last_segments(0) >= 1 and lib.oss_scan_last_segments(1) >= 1


def test_cpu_tensors_are_rejected_not_silently_computed():
    """The product has no CPU path: the op only has a GPU kernel (cf. TORCH_CHECK(u.is_cuda()),
    cus/selective_scan.cpp:174)."""
    u = torch.zeros(1, 4, 8)
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        vmambair_amd.selective_scan_fwd(u, u, torch.zeros(4, 2), torch.zeros(1, 1, 2, 8), torch.zeros(1, 1, 2, 8),
                                        None, None, True, 1)
    with pytest.raises(RuntimeError):
        vmambair_amd.selective_scan_fwd(u.double(), u.double(), torch.zeros(4, 2), torch.zeros(1, 1, 2, 8),
                                        torch.zeros(1, 1, 2, 8), None, None, True, 1)


def test_drop_in_module_surface():
    import selective_scan_cuda_core as m
    assert callable(m.fwd) and callable(m.bwd)


def test_compiled_torch_boundary_is_built_and_registers_its_ops():
    """lib/libvmambair_torch.so (csrc_host/oss_torch_host.cpp) loads without a GPU and defines the two operators with the
    mutated-argument annotation; no compute call here"""
    from vmambair_amd import _host
    assert os.path.exists(_build.HOST_LIB), "run __graft_entry__.build() first"
    assert _host.mode() == "c++"
    ops = _host.ops()
    s = str(ops.scan_bwd.default._schema)
    assert "Tensor(a!)? dbc_into" in s and str(ops.scan_fwd.default._schema).endswith("-> Tensor[]")


def test_missing_torch_boundary_is_a_hard_error(monkeypatch, tmp_path):
    """no fallback: without lib/libvmambair_torch.so the scan ops raise and name the build command, like _capi.load()"""
    from vmambair_amd import _host
    monkeypatch.setattr(_host, "_ops", None)          # restored afterwards: later tests load normally
    monkeypatch.setattr(_build, "HOST_LIB", str(tmp_path / "libvmambair_torch.so"))
    with pytest.raises(RuntimeError, match=r"libvmambair_torch\.so is missing.*__graft_entry__ as g; g\.build\(\)"):
        _host.ops()
    with pytest.raises(RuntimeError, match="is missing"):
        _host.mode()
    assert _host._ops is None


def test_stale_torch_boundary_is_refused_before_it_is_loaded(monkeypatch):
    """a host library compiled against another revision of include/vmambair_oss.h raises with abi_mismatch()'s reason and is
    never handed to torch.ops.load_library"""
    from vmambair_amd import _host
    loaded = []
    monkeypatch.setattr(_host, "_ops", None)
    monkeypatch.setattr(_host, "abi_mismatch", lambda: "compiled against another revision (test)")
    monkeypatch.setattr(torch.ops, "load_library", loaded.append)
    with pytest.raises(RuntimeError, match=r"compiled against another revision \(test\)"):
        _host.ops()
    assert loaded == [] and _host._ops is None
    monkeypatch.undo()
    assert _host.abi_mismatch() is None and hasattr(_host.ops(), "scan_fwd")


def test_shape_rules_of_the_fused_kernels_are_pure_host_queries():
    """which shapes the round-3 fused forms take (no GPU needed: the rules live in the library, the Python layer only asks)"""
    lib = _capi.load()
    BF16, F16, F32 = 2, 1, 0
    # depth-wise conv + silu (1 plane per workgroup) / + gelu gate (2 planes): 16-bit, W % 8 == 0, planes in LDS
    assert lib.oss_dwconv3x3_fused_ok(BF16, 64, 64, 1) == 1 and lib.oss_dwconv3x3_fused_ok(F16, 128, 128, 2) == 1
    # (round 4) float I/O too -- planes of twice the bytes: 64 x 64 gate fits, 160 x 160 gate (207 KiB) does not
    assert lib.oss_dwconv3x3_fused_ok(F32, 64, 64, 1) == 1 and lib.oss_dwconv3x3_fused_ok(F32, 64, 64, 2) == 1
    assert lib.oss_dwconv3x3_fused_ok(F32, 160, 160, 1) == 1 and lib.oss_dwconv3x3_fused_ok(F32, 160, 160, 2) == 0
    assert lib.oss_dwconv3x3_flat2_ok(F32, 64, 64) == 1 and lib.oss_dwconv3x3_flat2_ok(BF16, 12, 64) == 0 and lib.oss_dwconv3x3_flat2_ok(BF16, 16, 160) == 0
    # (round 4) rows whose W / 8 lane groups straddle waves are taken too (EDGE instantiations): RealSR's 160-wide tiles, W = 24
    assert lib.oss_dwconv3x3_fused_ok(F16, 160, 160, 1) == 1 and lib.oss_dwconv3x3_fused_ok(F16, 160, 160, 2) == 1
    assert lib.oss_dwconv3x3_fused_ok(BF16, 16, 24, 2) == 1 and lib.oss_dwconv3x3_fused_ok(BF16, 16, 20, 2) == 0
    assert lib.oss_dwconv3x3_fused_ok(BF16, 256, 256, 1) == 1 and lib.oss_dwconv3x3_fused_ok(BF16, 256, 256, 2) == 0   # 129 / 258 KiB
    assert lib.oss_dwconv3x3_fused_ok(BF16, 64, 64, 3) == 0
    # LayerNorm inside the 1x1 convolution: cin % 16 == 0, cin <= 192, pixels % 128 == 0
    assert lib.oss_ln_conv1x1_ok(BF16, 192, 96, 4096) == 1 and lib.oss_ln_conv1x1_ok(F16, 510, 96, 25600) == 1
    assert lib.oss_ln_conv1x1_ok(BF16, 768, 384, 1024) == 0         # level 4 of the UNet: K = 384
    assert lib.oss_ln_conv1x1_ok(BF16, 192, 96, 4000) == 0 and lib.oss_ln_conv1x1_ok(F32, 192, 96, 4096) == 0
    assert lib.oss_ln_conv1x1_ok(BF16, 254, 127, 4096) == 0
    # input gradient + LayerNorm backward: cin <= 128, 2 cin <= cout <= 192
    assert lib.oss_conv1x1_dgrad_ln_bwd_ok(BF16, 192, 96, 4096, 8) == 1 and lib.oss_conv1x1_dgrad_ln_bwd_ok(F16, 96, 48, 1024, 1) == 1
    assert lib.oss_conv1x1_dgrad_ln_bwd_ok(BF16, 510, 96, 4096, 8) == 0    # project_in: the wave-level kernel + its own LayerNorm launch
    assert lib.oss_conv1x1_dgrad_ln_bwd_ok(BF16, 96, 96, 4096, 8) == 0     # fewer than 2 cin rows to park x and the skip gradient in
    assert lib.oss_conv1x1_dgrad_ln_bwd_ok(BF16, 384, 192, 1024, 8) == 0
    n = lib.oss_conv1x1_dgrad_ln_bwd_partial_floats(8, 96, 4096)
    assert n == 8 * (4096 // 64) * 2 * 96
    assert lib.oss_conv1x1_dgrad_ln_bwd_partial_floats(0, 96, 4096) == 0


# every *_ok query that takes an oss_dtype, with arguments one of the element types answers 1 for
_DTYPE_PREDICATES = {
    "oss_scan_fused_dt_ok": (2, 96, 38, 6, 16, 4096),
    "oss_dwconv3x3_fused_ok": (64, 64, 1),
    "oss_dwgate_fwd_ok": (64, 64),
    "oss_effn_fwd_ok": (48, 127, 64, 64),
    "oss_dwconv3x3_flat2_ok": (64, 64),
    "oss_ln_conv1x1_ok": (192, 96, 4096),
    "oss_conv1x1_dgrad_ln_bwd_ok": (192, 96, 4096, 8),
    "oss_proj_rows_optional_ok": (2, 96, 38, 6, 4096),
    "oss_conv3x3_thin_ok": (3, 48, 16, 16),
    "oss_conv3x3_dense_ok": (32, 24, 8, 8),
    "oss_image_metrics_ok": (3, 32, 32, 4, 0),
}


def test_dtype_predicates_refuse_what_is_no_element_type():
    """one decoder of ``oss_dtype`` (``io_dispatch`` in csrc/oss_host.h): ``OSS_F32_BF16X3`` (3, a selector of the six GEMM-shaped
    entry points) and an out-of-range value (7) are no element type to any ``*_ok`` query -- none reads them as a 16-bit type"""
    lib = _capi.load()
    hdr = _stripped_header()
    declared = set(re.findall(r"\bint\s+(oss_\w+_ok)\s*\(\s*oss_dtype\b", hdr))
    assert declared == set(_DTYPE_PREDICATES), declared ^ set(_DTYPE_PREDICATES)
    assert _capi.OSS_F32_BF16X3 == 3
    for name, args in _DTYPE_PREDICATES.items():
        fn = getattr(lib, name)
        assert fn(_capi.OSS_BF16, *args) == 1, name      # the arguments are a shape the query takes ...
        assert fn(3, *args) == 0 and fn(7, *args) == 0, name   # ... so the 0 is the dtype's
        assert fn(-1, *args) == 0, name
