"""The host plan of the selective-scan launches (csrc/oss_scan_plan.h) through ``oss_scan_fwd_describe`` /
``oss_scan_bwd_describe`` (no GPU): what a call would launch is integer arithmetic on the parameter block, and three pieces of it
must agree -- the workspace size queries, the carving of the workspace and the carry slots the segment split may use.  The blocks
carry stand-in addresses where only a pointer's presence matters; nothing is launched and nothing is dereferenced."""
import ctypes
import itertools

import pytest

from vmambair_amd import _capi

OK, ERR_SHAPE, ERR_WORKSPACE = 0, _capi._K["OSS_ERR_SHAPE"], _capi._K["OSS_ERR_WORKSPACE"]
Launch = _capi._HDR.structs["oss_scan_launch"]
LDS_MAX = 160 * 1024
PTR = 0x10000          # a stand-in address
HUGE = 1 << 60

BATCHES = (1, 2, 8)
DIM_GROUPS = ((24, 2), (26, 2), (48, 4), (384, 4), (96, 1), (12, 1), (7, 7))
SEQLENS = (1, 255, 257, 512, 513, 1061, 2085, 3000, 4096, 6600, 16384, 33000)
DSTATES = (1, 5, 16, 40, 64)
FWD_VARIANTS = (0, 1, 2, 3, 4, 6)
BWD_VARIANTS = (1, 10, 11, 12, 13)
SEG_REQUESTS = (-1, 0, 2, 3, 7, 64)
CARRY_SPLITS = (0, 1, 2, 4, 64)
FWD_KERNELS = {0: (8, 512), 1: (16, 512), 2: (16, 256), 3: (8, 1024), 4: (4, 256), 6: (12, 1024)}   # variant: rows, chunk
BWD_KERNELS = {1: (4, 256), 10: (12, 512), 11: (8, 512), 12: (6, 512), 13: (4, 512)}


def ceil(a, b):
    return -(-a // b)


def fwd_query(B, dim, L, N, G):
    S = min(64, ceil(L, 256))
    return 8 * B * dim * N * S if S > 1 else 0


def bwd_query(B, dim, L, N, G):
    S = min(64, max(1, ceil(L, 512)))
    return 4 * (B * G * ceil(dim // G, 4) * (2 * N + 8) * L + B * S * dim * (N + 10) + (2 * B * dim * N * S if S > 1 else 0))


def bwd_need(B, dim, L, N, G, rows, rp, n_seg, slots):
    """bytes of the backward's workspace for one launch shape: row-tile partials, weight partials per (batch, segment), carry pairs"""
    return 4 * (B * G * ceil(dim // G, rows) * (2 * N + rp) * L + B * n_seg * dim * (N + 2 + (8 if rp else 0)) +
                (2 * B * dim * N * slots if n_seg > 1 else 0))


@pytest.fixture
def lib():
    lib = _capi.load()
    yield lib
    lib.oss_scan_set_variant(-1, -1)
    lib.oss_scan_set_segments(-1, -1)
    lib.oss_scan_set_carry_split(0)


def fwd_block(B, dim, L, N, G, variant=None, ws_bytes=HUGE, dtw=False, rank=8, ws=True):
    p = _capi.ScanFwdParams()
    p.batch, p.dim, p.seqlen, p.dstate, p.n_groups = B, dim, L, N, G
    p.rev_group_start = G
    p.workspace, p.workspace_bytes = (PTR if ws else None), ws_bytes
    if dtw:
        p.dt_weight, p.dt_rank = PTR, rank
    if variant is not None:
        p.tune_variant = variant + 1
    return p


def bwd_block(B, dim, L, N, G, variant=None, ws_bytes=HUGE, dtw=False, rank=8, hs=False, partials=0):
    q = _capi.ScanBwdParams()
    f = q.f
    f.batch, f.dim, f.seqlen, f.dstate, f.n_groups = B, dim, L, N, G
    f.rev_group_start = G
    q.workspace, q.workspace_bytes = PTR, ws_bytes
    if dtw:
        f.dt_weight, f.dt_rank = PTR, rank
        q.ddt, q.ddt_weight = PTR, PTR
    if hs:
        f.hs = PTR
    if variant is not None:
        q.tune_variant = variant + 1
    q.tune_partials = partials
    return q


def check_segments(o, L, req, fused, can_segment):
    """the five segment numbers of a described launch, and the segment count against the request"""
    n_chunks = ceil(L, o.chunk)
    n, cps, csub, ccps = o.segments, o.chunks_per_segment, o.carry_pieces, o.chunks_per_piece
    assert (n - 1) * cps < n_chunks <= n * cps
    assert ccps == ceil(cps, csub) and (csub - 1) * ccps < cps
    assert n * csub <= min(n_chunks, 64)
    if fused or not can_segment or req in (0, 1) or n_chunks < 2:
        assert n == 1
    elif req > 1:
        want = min(req, n_chunks, 64)          # before the rounding to whole chunks per segment
        assert n == ceil(n_chunks, ceil(n_chunks, want))
    elif o.workgroups >= 256:
        assert n == 1
    if n == 1:
        assert csub == 1 and cps == n_chunks


@pytest.mark.parametrize("dim,G", DIM_GROUPS)
def test_forward_plan_fits_the_queried_workspace(lib, dim, G):
    """every forward variant, segment request and carry split at every shape: a workspace of exactly the size the query returns
    runs the plan an unlimited one would, inside the LDS, with consistent segment numbers"""
    desc, o, full = lib.oss_scan_fwd_describe, Launch(), Launch()
    for req, split in itertools.product(SEG_REQUESTS, CARRY_SPLITS):
        lib.oss_scan_set_segments(req, req)
        lib.oss_scan_set_carry_split(split)
        for B, L, N, v, dtw in itertools.product(BATCHES, SEQLENS, DSTATES, FWD_VARIANTS, (False, True)):
            query = lib.oss_scan_fwd_workspace_bytes(B, dim, L, N, G)
            assert query == fwd_query(B, dim, L, N, G)
            p = fwd_block(B, dim, L, N, G, v, query, dtw)
            assert desc(ctypes.byref(p), _capi.OSS_BF16, ctypes.byref(o)) == OK
            p.workspace_bytes = HUGE
            assert desc(ctypes.byref(p), _capi.OSS_BF16, ctypes.byref(full)) == OK
            assert bytes(o) == bytes(full), "the queried workspace made the launch fall back"
            assert o.workspace_bytes <= query and o.lds_bytes <= LDS_MAX
            assert o.variant == v and (o.rows_per_workgroup, o.chunk) == FWD_KERNELS[v] and o.fused_delta == dtw
            assert o.workgroups == B * G * ceil(dim // G, o.rows_per_workgroup)
            assert o.workspace_bytes == (8 * B * dim * N * o.segments * o.carry_pieces if o.segments > 1 else 0)
            check_segments(o, L, req, dtw, True)
            if split > 0:
                assert o.carry_pieces <= split


@pytest.mark.parametrize("dim,G", DIM_GROUPS)
def test_backward_plan_fits_the_queried_workspace(lib, dim, G):
    desc, o, full = lib.oss_scan_bwd_describe, Launch(), Launch()
    for req, split in itertools.product(SEG_REQUESTS, CARRY_SPLITS):
        lib.oss_scan_set_segments(req, req)
        lib.oss_scan_set_carry_split(split)
        for B, L, N, v, dtw in itertools.product(BATCHES, SEQLENS, DSTATES, BWD_VARIANTS, (False, True)):
            query = lib.oss_scan_bwd_workspace_bytes(B, dim, L, N, G)
            assert query == bwd_query(B, dim, L, N, G)
            q = bwd_block(B, dim, L, N, G, v, query, dtw)
            assert desc(ctypes.byref(q), _capi.OSS_BF16, ctypes.byref(o)) == OK
            q.workspace_bytes = HUGE
            assert desc(ctypes.byref(q), _capi.OSS_BF16, ctypes.byref(full)) == OK
            assert bytes(o) == bytes(full), "the queried workspace made the launch fall back"
            assert o.workspace_bytes <= query and o.lds_bytes <= LDS_MAX
            kernel = 13 if dtw and v < 10 else v              # the fused-delta form runs the round-2 kernels only
            assert o.variant == v and (o.rows_per_workgroup, o.chunk) == BWD_KERNELS[kernel] and o.fused_delta == dtw
            assert o.workgroups == B * G * ceil(dim // G, o.rows_per_workgroup)
            assert o.workspace_bytes == bwd_need(B, dim, L, N, G, o.rows_per_workgroup, 8 if dtw else 0, o.segments,
                                                 o.segments * o.carry_pieces)
            check_segments(o, L, req, dtw, kernel >= 10)
            if split > 0:
                assert o.carry_pieces <= split


def test_size_queries_refuse_what_they_always_refused(lib):
    for fn in (lib.oss_scan_fwd_workspace_bytes, lib.oss_scan_bwd_workspace_bytes):
        assert fn(2, 24, 3000, 16, 5) == 0, "dim % groups"
        for bad in ((0, 24, 3000, 16, 2), (2, 0, 3000, 16, 2), (2, 24, 0, 16, 2), (2, 24, 3000, 0, 2), (2, 24, 3000, 16, 0),
                    (-1, 24, 3000, 16, 2), (2, 24, -5, 16, 2)):
            assert fn(*bad) == 0
    assert lib.oss_scan_fwd_workspace_bytes(2, 24, 256, 16, 2) == 0 and lib.oss_scan_fwd_workspace_bytes(2, 24, 257, 16, 2) > 0


@pytest.mark.parametrize("B,dim,G,L,N", [(2, 26, 2, 16384, 16), (1, 384, 4, 16384, 16), (2, 24, 2, 33000, 5), (1, 12, 1, 33000, 64)])
@pytest.mark.parametrize("req", [3, 7])
def test_workspace_ladder(lib, B, dim, G, L, N, req):
    """finer carry split -> csub = 1 -> unsegmented -> (backward) OSS_ERR_WORKSPACE, each at exactly the bytes the step needs"""
    lib.oss_scan_set_segments(req, req)
    o = Launch()

    def fwd(ws_bytes, ws=True, split=0):
        p = fwd_block(B, dim, L, N, G, 6, ws_bytes, ws=ws)
        p.tune_carry_split = split
        return lib.oss_scan_fwd_describe(ctypes.byref(p), _capi.OSS_F32, ctypes.byref(o)), o.segments, o.carry_pieces, o.workspace_bytes

    def bwd(ws_bytes, split=0):
        q = bwd_block(B, dim, L, N, G, 10, ws_bytes)
        q.f.tune_carry_split = split
        return lib.oss_scan_bwd_describe(ctypes.byref(q), _capi.OSS_F32, ctypes.byref(o)), o.segments, o.carry_pieces, o.workspace_bytes

    for run, unsegmented in ((fwd, 0), (bwd, bwd_need(B, dim, L, N, G, 12, 0, 1, 0))):
        rc, n, csub, need = run(HUGE, split=4)
        assert rc == OK and n > 1 and csub > 1, "the case must exercise the finer split"
        coarse = run(HUGE, split=1)
        assert coarse[:3] == (OK, n, 1) and unsegmented < coarse[3] < need
        assert run(need, split=4) == (OK, n, csub, need)
        assert run(need - 1, split=4) == coarse, "one byte short of the finer split: same segments, csub = 1"
        assert run(coarse[3], split=4) == coarse
        assert run(coarse[3] - 1, split=4) == (OK, 1, 1, unsegmented), "one byte short of the segments' own slots: one segment"
        assert run(unsegmented, split=4) == (OK, 1, 1, unsegmented)
    assert bwd(unsegmented - 1)[0] == ERR_WORKSPACE
    assert fwd(HUGE, ws=False)[:3] == (OK, 1, 1), "no forward workspace: one segment, not an error"
    assert fwd(0)[:3] == (OK, 1, 1)


def test_remaps(lib):
    o = Launch()
    bdesc = lambda q, io=_capi.OSS_BF16: lib.oss_scan_bwd_describe(ctypes.byref(q), io, ctypes.byref(o))
    # round-2 variants keep one lane per state: dstate > 64 runs the 4-row, 256-step round-1 kernel, unsegmented
    lib.oss_scan_set_segments(4, 4)
    for v in (10, 11, 12, 13):
        assert bdesc(bwd_block(1, 24, 4096, 72, 2, v)) == OK
        assert (o.variant, o.rows_per_workgroup, o.chunk, o.segments, o.lane_states) == (v, 4, 256, 1, 0)
    assert bdesc(bwd_block(1, 24, 4096, 64, 2, 11)) == OK and (o.rows_per_workgroup, o.chunk, o.segments) == (8, 512, 4)
    assert bdesc(bwd_block(1, 24, 4096, 64, 2, 1)) == OK and (o.rows_per_workgroup, o.chunk, o.segments) == (4, 256, 1)
    # dt_weight: round-2 kernels only
    for v in (0, 1, 5, 9):
        assert bdesc(bwd_block(2, 48, 700, 16, 2, v, dtw=True, rank=5)) == OK
        assert (o.variant, o.rows_per_workgroup, o.chunk, o.fused_delta, o.segments) == (v, 4, 512, 1, 1)
    assert bdesc(bwd_block(2, 48, 700, 72, 2, 13, dtw=True)) == ERR_SHAPE
    assert bdesc(bwd_block(2, 48, 700, 16, 2, 13, dtw=True, rank=0)) == ERR_SHAPE
    assert bdesc(bwd_block(2, 48, 700, 16, 2, 13, dtw=True, rank=9)) == ERR_SHAPE
    q = bwd_block(2, 48, 700, 16, 2, 13, dtw=True)
    q.ddt = None
    assert bdesc(q) == ERR_SHAPE
    p = fwd_block(2, 48, 700, 16, 2, 3, dtw=True, rank=9)
    assert lib.oss_scan_fwd_describe(ctypes.byref(p), _capi.OSS_F32, ctypes.byref(o)) == ERR_SHAPE
    # the forward tiles of variant 6 + per-row carries do not fit the LDS at dstate 250: 4 rows, 256-step chunks
    p = fwd_block(1, 24, 2000, 250, 2, 6)
    assert lib.oss_scan_fwd_describe(ctypes.byref(p), _capi.OSS_F32, ctypes.byref(o)) == OK
    assert (o.variant, o.rows_per_workgroup, o.chunk) == (6, 4, 256) and o.lds_bytes <= LDS_MAX
    p = fwd_block(1, 24, 2000, 64, 2, 6)
    assert lib.oss_scan_fwd_describe(ctypes.byref(p), _capi.OSS_F32, ctypes.byref(o)) == OK and (o.rows_per_workgroup, o.chunk) == (12, 1024)
    # bf16 partials: bf16 I/O, no dt_weight, no hs, round-2 kernels
    lib.oss_scan_set_segments(-1, -1)
    for io, kw, want in ((_capi.OSS_BF16, {}, 1), (_capi.OSS_F16, {}, 0), (_capi.OSS_F32, {}, 0), (_capi.OSS_BF16, {"dtw": True}, 0),
                         (_capi.OSS_BF16, {"hs": True}, 0), (_capi.OSS_BF16, {"variant": 1}, 0)):
        assert bdesc(bwd_block(2, 24, 2085, 16, 2, **{"variant": 11, **kw}, partials=2), io) == OK
        assert o.bf16_partials == want, (io, kw)
    assert bdesc(bwd_block(2, 24, 2085, 16, 2, 11, partials=1)) == OK and o.bf16_partials == 0
    # lane states: not with dt_weight, not the round-1 kernel
    for kw, want in (({}, 1), ({"dtw": True}, 0), ({"variant": 1}, 0)):
        assert bdesc(bwd_block(2, 24, 2085, 16, 2, **{"variant": 11, **kw}, hs=True)) == OK and o.lane_states == want, kw
    assert bdesc(bwd_block(2, 24, 2085, 72, 2, 11, hs=True)) == OK and o.lane_states == 0
    # an empty call launches nothing; shape errors are the entry points'
    assert bdesc(bwd_block(0, 24, 2085, 16, 2)) == OK and (o.variant, o.workgroups, o.segments) == (-1, 0, 0)
    assert bdesc(bwd_block(2, 24, 2085, 16, 5)) == ERR_SHAPE
    assert bdesc(bwd_block(2, 24, 2085, 300, 2)) == _capi._K["OSS_ERR_DSTATE"]
    assert lib.oss_scan_bwd_describe(None, _capi.OSS_BF16, ctypes.byref(o)) == _capi._K["OSS_ERR_NULL"]
    assert bdesc(bwd_block(2, 24, 2085, 16, 2), _capi.OSS_F32_BF16X3) == ERR_SHAPE


def test_segment_heuristic_fills_idle_cus_only(lib):
    """the cases tests/test_scan_gpu.py asserts after real launches: bf16, dstate 16, 4 groups, heuristics throughout"""
    o = Launch()
    for (B, dim, L), cut in (((8, 384, 4096), False), ((1, 384, 16384), True), ((4, 192, 16384), True)):
        p = fwd_block(B, dim, L, 16, 4, ws_bytes=lib.oss_scan_fwd_workspace_bytes(B, dim, L, 16, 4))
        assert lib.oss_scan_fwd_describe(ctypes.byref(p), _capi.OSS_BF16, ctypes.byref(o)) == OK
        fwd_segments = o.segments
        q = bwd_block(B, dim, L, 16, 4, ws_bytes=lib.oss_scan_bwd_workspace_bytes(B, dim, L, 16, 4))
        assert lib.oss_scan_bwd_describe(ctypes.byref(q), _capi.OSS_BF16, ctypes.byref(o)) == OK
        assert (fwd_segments > 1, o.segments > 1) == (cut, cut), (B, dim, L, fwd_segments, o.segments)
