"""Host side of the pre-packed weight images of the 1x1 convolutions (no GPU): the size queries of include/vmambair_oss.h, the
table rows ``oss_conv1x1_pack_fill`` writes, and the set / clear behaviour of the registry in ops/pointwise.py."""
import ctypes

import pytest
import torch

from vmambair_amd import _capi
from vmambair_amd.ops import pointwise as pw

SHAPES = [(96, 255), (48, 127), (33, 193), (254, 48), (96, 48), (5, 17), (1, 1), (32, 16), (33, 17), (510, 96)]


def _ceil(a, b):
    return (a + b - 1) // b


@pytest.mark.parametrize("cout,cin", SHAPES)
def test_image_size_queries(cout, cin):
    """ceil(M / 32) * ceil(K / 16) * 1024 bytes: forward M = cout, K = cin; input gradient M = cin, K = cout"""
    lib = _capi.load()
    assert lib.oss_conv1x1_fwd_image_bytes(cout, cin) == _ceil(cout, 32) * _ceil(cin, 16) * 1024
    assert lib.oss_conv1x1_dgrad_image_bytes(cout, cin) == _ceil(cin, 32) * _ceil(cout, 16) * 1024
    assert lib.oss_conv1x1_fwd_image_bytes(0, cin) == 0 and lib.oss_conv1x1_dgrad_image_bytes(cout, -1) == 0
    # a table row covers 256 pieces of 16 bytes of ONE image
    rows = _ceil(lib.oss_conv1x1_fwd_image_bytes(cout, cin), 4096) + _ceil(lib.oss_conv1x1_dgrad_image_bytes(cout, cin), 4096)
    assert lib.oss_conv1x1_pack_rows(cout, cin) == rows and lib.oss_conv1x1_pack_rows(cout, 0) == 0


def test_pack_fill_writes_the_rows_of_both_images():
    lib = _capi.load()
    cout, cin = 33, 193
    rb = lib.oss_conv1x1_pack_row_bytes()
    n = lib.oss_conv1x1_pack_rows(cout, cin)
    assert rb == 32 and n == 7 + 6     # 2 x 13 units of 1 KiB -> 7 rows; 7 x 3 units -> 6 rows
    buf = (ctypes.c_uint8 * (rb * n + 8))(*([0xee] * (rb * n + 8)))
    w, fimg, dimg = 0x1000, 0x200000, 0x300000      # stand-in addresses: the call only writes them down
    assert lib.oss_conv1x1_pack_fill(ctypes.addressof(buf), w, fimg, dimg, cout, cin) == n
    assert bytes(buf[rb * n:]) == b"\xee" * 8, "wrote past its rows"

    class Row(ctypes.Structure):
        _fields_ = [("w", ctypes.c_uint64), ("img", ctypes.c_uint64), ("M", ctypes.c_int), ("K", ctypes.c_int), ("wt", ctypes.c_int),
                    ("first", ctypes.c_int)]
    rows = (Row * n).from_buffer(buf)
    got = [(r.w, r.img, r.M, r.K, r.wt, r.first) for r in rows]
    want = [(w, fimg, cout, cin, 0, 256 * i) for i in range(7)] + [(w, dimg, cin, cout, 1, 256 * i) for i in range(6)]
    assert got == want
    assert lib.oss_conv1x1_pack_fill(ctypes.addressof(buf), w, fimg + 8, dimg, cout, cin) == -2      # OSS_ERR_SHAPE: misaligned image
    assert lib.oss_conv1x1_pack_fill(ctypes.addressof(buf), w, 0, dimg, cout, cin) == -1             # OSS_ERR_NULL


def test_registry_set_and_clear():
    w = torch.zeros(6, 10)
    other = torch.zeros(6, 10)
    fimg, dimg = torch.zeros(1024, dtype=torch.uint8), torch.zeros(1024, dtype=torch.uint8)
    assert pw.packed_images_active() == 0 and pw._packed_image(w, torch.bfloat16, 0) == 0
    pw.set_packed_images({w.data_ptr(): (6, 10, torch.bfloat16, fimg, dimg)})
    try:
        assert pw.packed_images_active() == 1
        assert pw._packed_image(w, torch.bfloat16, 0) == fimg.data_ptr() and pw._packed_image(w, torch.bfloat16, 1) == dimg.data_ptr()
        assert pw._packed_image(w, torch.float16, 0) == 0            # packed for another type
        assert pw._packed_image(other, torch.bfloat16, 0) == 0       # another storage
        assert pw._packed_image(w.view(10, 6), torch.bfloat16, 0) == 0   # same storage, another shape
        pw.set_packed_images({})                                    # a new set replaces the old one
        assert pw.packed_images_active() == 0 and pw._packed_image(w, torch.bfloat16, 0) == 0
        pw.set_packed_images({w.data_ptr(): (6, 10, torch.bfloat16, fimg, dimg)})
    finally:
        pw.clear_packed_images()
    assert pw.packed_images_active() == 0 and pw._packed_image(w, torch.bfloat16, 1) == 0
