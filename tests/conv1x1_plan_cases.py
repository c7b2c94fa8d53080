"""The instantiations the 1x1-convolution launchers can emit (csrc/oss_conv1x1_plan.h), shared by tests/test_conv1x1_plan_host.py,
tests/test_conv1x1_plan_gpu.py and tools/conv1x1_launch_dump.py.

A launch is named by the tuple ``(family, KS, MT, WT, WVEC, RES, PF, WIMG, PT, X3)`` of ``oss_conv1x1_launch`` (a template argument
the family does not have is 0; PT = pixels per workgroup, a template argument of the workgroup-level kernel only).  ``EXPECTED``
is written down from the launchers' ``switch`` statements, not from what the library answers; ``SMALLEST`` gives, per tuple, the
smallest call of the host test's grid that reaches it:
``(io, input_gradient, B, M, K, P, residual, image, w address & 15, x address & 15, xsk - P, (wg on, wg pixels))`` with
M = output rows and K = contracted channels of the product (forward: cout, cin; input gradient: cin, cout)."""
WG, PAIR, PAIRW, PAIRK, REUSE, GENERIC, F32_TILE64, F32_TILE32, F32_SPLITK = range(9)
FAMILY_NAMES = ("wg", "pair", "pairw", "pairk", "reuse", "generic", "f32_tile64", "f32_tile32", "f32_splitk")
FIELDS = ("family", "ks", "mt", "wt", "wvec", "res", "pf", "wimg", "pt", "x3")

# weight forms of the pixel-pair kernels without an image: (WT, WVEC) = transposed | 16-byte rows | per element
_FORMS = ((1, 0), (0, 1), (0, 0))
EXPECTED = set()
# wg: KS x WT x PT x WIMG, PF = KS <= 6, never RES
EXPECTED |= {(WG, ks, 0, wt, 0, 0, int(ks <= 6), img, pt, 0) for ks in (1, 2, 3, 4, 6, 8, 12) for wt in (0, 1) for pt in (64, 128) for img in (0, 1)}
# pair: KS x form x RES with PF = KS <= 6; from an image (WT = WVEC = 0) PF = KS <= 8
EXPECTED |= {(PAIR, ks, 0, wt, wv, res, int(ks <= 6), 0, 256, 0) for ks in (3, 6, 8, 12) for wt, wv in _FORMS for res in (0, 1)}
EXPECTED |= {(PAIR, ks, 0, 0, 0, res, int(ks <= 8), 1, 256, 0) for ks in (3, 6, 8, 12) for res in (0, 1)}
# pairk: KS = 8, MT x (form | image)
EXPECTED |= {(PAIRK, 8, mt, wt, wv, 0, 0, 0, 256, 0) for mt in (1, 2, 3) for wt, wv in _FORMS}
EXPECTED |= {(PAIRK, 8, mt, 0, 0, 0, 0, 1, 256, 0) for mt in (1, 2, 3)}
EXPECTED |= {(PAIRW, 0, 0, 0, 0, 0, 0, 0, 256, 0), (GENERIC, 0, 0, 0, 0, 0, 0, 0, 128, 0)}
EXPECTED |= {(REUSE, ks, 0, wt, 0, 0, 0, 0, 128, 0) for ks in (6, 12) for wt in (0, 1)}
EXPECTED |= {(fam, 0, mt, 0, 0, 0, 0, 0, 128, x3) for fam, mt in ((F32_TILE64, 2), (F32_TILE32, 1), (F32_SPLITK, 1)) for x3 in (0, 1)}
# Built (as they always were) but beyond every entry point: the input gradient has no residual, so WT meets RES only in the
# forward of a 1 -> 1 convolution, whose weight matrix reads the same both ways (KS = 3).
UNREACHABLE = {(PAIR, ks, 0, 1, 0, 1, int(ks <= 6), 0, 256, 0) for ks in (6, 8, 12)}
EXPECTED -= UNREACHABLE

SMALLEST = {
    (0, 1, 0, 0, 0, 0, 1, 0, 64, 0): ('bf16', 0, 1, 1, 16, 128, 0, 0, 0, 0, 0, (1, 0)),
    (0, 1, 0, 0, 0, 0, 1, 0, 128, 0): ('bf16', 0, 1, 1, 16, 128, 0, 0, 0, 0, 0, (1, 128)),
    (0, 1, 0, 0, 0, 0, 1, 1, 64, 0): ('bf16', 0, 1, 1, 16, 128, 0, 1, 0, 0, 0, (1, 0)),
    (0, 1, 0, 0, 0, 0, 1, 1, 128, 0): ('bf16', 0, 1, 1, 16, 128, 0, 1, 0, 0, 0, (1, 128)),
    (0, 1, 0, 1, 0, 0, 1, 0, 64, 0): ('bf16', 1, 1, 1, 16, 128, 0, 0, 0, 0, 0, (1, 0)),
    (0, 1, 0, 1, 0, 0, 1, 0, 128, 0): ('bf16', 1, 1, 1, 16, 128, 0, 0, 0, 0, 0, (1, 128)),
    (0, 1, 0, 1, 0, 0, 1, 1, 64, 0): ('bf16', 1, 1, 1, 16, 128, 0, 1, 0, 0, 0, (1, 0)),
    (0, 1, 0, 1, 0, 0, 1, 1, 128, 0): ('bf16', 1, 1, 1, 16, 128, 0, 1, 0, 0, 0, (1, 128)),
    (0, 2, 0, 0, 0, 0, 1, 0, 64, 0): ('bf16', 0, 1, 1, 32, 128, 0, 0, 0, 0, 0, (1, 0)),
    (0, 2, 0, 0, 0, 0, 1, 0, 128, 0): ('bf16', 0, 1, 1, 32, 128, 0, 0, 0, 0, 0, (1, 128)),
    (0, 2, 0, 0, 0, 0, 1, 1, 64, 0): ('bf16', 0, 1, 1, 32, 128, 0, 1, 0, 0, 0, (1, 0)),
    (0, 2, 0, 0, 0, 0, 1, 1, 128, 0): ('bf16', 0, 1, 1, 32, 128, 0, 1, 0, 0, 0, (1, 128)),
    (0, 2, 0, 1, 0, 0, 1, 0, 64, 0): ('bf16', 1, 1, 1, 32, 128, 0, 0, 0, 0, 0, (1, 0)),
    (0, 2, 0, 1, 0, 0, 1, 0, 128, 0): ('bf16', 1, 1, 1, 32, 128, 0, 0, 0, 0, 0, (1, 128)),
    (0, 2, 0, 1, 0, 0, 1, 1, 64, 0): ('bf16', 1, 1, 1, 32, 128, 0, 1, 0, 0, 0, (1, 0)),
    (0, 2, 0, 1, 0, 0, 1, 1, 128, 0): ('bf16', 1, 1, 1, 32, 128, 0, 1, 0, 0, 0, (1, 128)),
    (0, 3, 0, 0, 0, 0, 1, 0, 64, 0): ('bf16', 0, 1, 1, 48, 128, 0, 0, 0, 0, 0, (1, 0)),
    (0, 3, 0, 0, 0, 0, 1, 0, 128, 0): ('bf16', 0, 1, 1, 48, 128, 0, 0, 0, 0, 0, (1, 128)),
    (0, 3, 0, 0, 0, 0, 1, 1, 64, 0): ('bf16', 0, 1, 1, 48, 128, 0, 1, 0, 0, 0, (1, 0)),
    (0, 3, 0, 0, 0, 0, 1, 1, 128, 0): ('bf16', 0, 1, 1, 48, 128, 0, 1, 0, 0, 0, (1, 128)),
    (0, 3, 0, 1, 0, 0, 1, 0, 64, 0): ('bf16', 1, 1, 1, 48, 128, 0, 0, 0, 0, 0, (1, 0)),
    (0, 3, 0, 1, 0, 0, 1, 0, 128, 0): ('bf16', 1, 1, 1, 48, 128, 0, 0, 0, 0, 0, (1, 128)),
    (0, 3, 0, 1, 0, 0, 1, 1, 64, 0): ('bf16', 1, 1, 1, 48, 128, 0, 1, 0, 0, 0, (1, 0)),
    (0, 3, 0, 1, 0, 0, 1, 1, 128, 0): ('bf16', 1, 1, 1, 48, 128, 0, 1, 0, 0, 0, (1, 128)),
    (0, 4, 0, 0, 0, 0, 1, 0, 64, 0): ('bf16', 0, 1, 1, 64, 128, 0, 0, 0, 0, 0, (1, 0)),
    (0, 4, 0, 0, 0, 0, 1, 0, 128, 0): ('bf16', 0, 1, 1, 64, 128, 0, 0, 0, 0, 0, (1, 128)),
    (0, 4, 0, 0, 0, 0, 1, 1, 64, 0): ('bf16', 0, 1, 1, 64, 128, 0, 1, 0, 0, 0, (1, 0)),
    (0, 4, 0, 0, 0, 0, 1, 1, 128, 0): ('bf16', 0, 1, 1, 64, 128, 0, 1, 0, 0, 0, (1, 128)),
    (0, 4, 0, 1, 0, 0, 1, 0, 64, 0): ('bf16', 1, 1, 1, 64, 128, 0, 0, 0, 0, 0, (1, 0)),
    (0, 4, 0, 1, 0, 0, 1, 0, 128, 0): ('bf16', 1, 1, 1, 64, 128, 0, 0, 0, 0, 0, (1, 128)),
    (0, 4, 0, 1, 0, 0, 1, 1, 64, 0): ('bf16', 1, 1, 1, 64, 128, 0, 1, 0, 0, 0, (1, 0)),
    (0, 4, 0, 1, 0, 0, 1, 1, 128, 0): ('bf16', 1, 1, 1, 64, 128, 0, 1, 0, 0, 0, (1, 128)),
    (0, 6, 0, 0, 0, 0, 1, 0, 64, 0): ('bf16', 0, 1, 1, 96, 128, 0, 0, 0, 0, 0, (1, 0)),
    (0, 6, 0, 0, 0, 0, 1, 0, 128, 0): ('bf16', 0, 1, 1, 96, 128, 0, 0, 0, 0, 0, (1, 128)),
    (0, 6, 0, 0, 0, 0, 1, 1, 64, 0): ('bf16', 0, 1, 1, 96, 128, 0, 1, 0, 0, 0, (1, 0)),
    (0, 6, 0, 0, 0, 0, 1, 1, 128, 0): ('bf16', 0, 1, 1, 96, 128, 0, 1, 0, 0, 0, (1, 128)),
    (0, 6, 0, 1, 0, 0, 1, 0, 64, 0): ('bf16', 1, 1, 1, 96, 128, 0, 0, 0, 0, 0, (1, 0)),
    (0, 6, 0, 1, 0, 0, 1, 0, 128, 0): ('bf16', 1, 1, 1, 96, 128, 0, 0, 0, 0, 0, (1, 128)),
    (0, 6, 0, 1, 0, 0, 1, 1, 64, 0): ('bf16', 1, 1, 1, 96, 128, 0, 1, 0, 0, 0, (1, 0)),
    (0, 6, 0, 1, 0, 0, 1, 1, 128, 0): ('bf16', 1, 1, 1, 96, 128, 0, 1, 0, 0, 0, (1, 128)),
    (0, 8, 0, 0, 0, 0, 0, 0, 64, 0): ('bf16', 0, 1, 1, 128, 128, 0, 0, 0, 0, 0, (1, 0)),
    (0, 8, 0, 0, 0, 0, 0, 0, 128, 0): ('bf16', 0, 1, 1, 128, 128, 0, 0, 0, 0, 0, (1, 128)),
    (0, 8, 0, 0, 0, 0, 0, 1, 64, 0): ('bf16', 0, 1, 1, 128, 128, 0, 1, 0, 0, 0, (1, 0)),
    (0, 8, 0, 0, 0, 0, 0, 1, 128, 0): ('bf16', 0, 1, 1, 128, 128, 0, 1, 0, 0, 0, (1, 128)),
    (0, 8, 0, 1, 0, 0, 0, 0, 64, 0): ('bf16', 1, 1, 1, 128, 128, 0, 0, 0, 0, 0, (1, 0)),
    (0, 8, 0, 1, 0, 0, 0, 0, 128, 0): ('bf16', 1, 1, 1, 128, 128, 0, 0, 0, 0, 0, (1, 128)),
    (0, 8, 0, 1, 0, 0, 0, 1, 64, 0): ('bf16', 1, 1, 1, 128, 128, 0, 1, 0, 0, 0, (1, 0)),
    (0, 8, 0, 1, 0, 0, 0, 1, 128, 0): ('bf16', 1, 1, 1, 128, 128, 0, 1, 0, 0, 0, (1, 128)),
    (0, 12, 0, 0, 0, 0, 0, 0, 64, 0): ('bf16', 0, 1, 1, 192, 128, 0, 0, 0, 0, 0, (1, 0)),
    (0, 12, 0, 0, 0, 0, 0, 0, 128, 0): ('bf16', 0, 1, 1, 192, 128, 0, 0, 0, 0, 0, (1, 128)),
    (0, 12, 0, 0, 0, 0, 0, 1, 64, 0): ('bf16', 0, 1, 1, 192, 128, 0, 1, 0, 0, 0, (1, 0)),
    (0, 12, 0, 0, 0, 0, 0, 1, 128, 0): ('bf16', 0, 1, 1, 192, 128, 0, 1, 0, 0, 0, (1, 128)),
    (0, 12, 0, 1, 0, 0, 0, 0, 64, 0): ('bf16', 1, 1, 1, 192, 128, 0, 0, 0, 0, 0, (1, 0)),
    (0, 12, 0, 1, 0, 0, 0, 0, 128, 0): ('bf16', 1, 1, 1, 192, 128, 0, 0, 0, 0, 0, (1, 128)),
    (0, 12, 0, 1, 0, 0, 0, 1, 64, 0): ('bf16', 1, 1, 1, 192, 128, 0, 1, 0, 0, 0, (1, 0)),
    (0, 12, 0, 1, 0, 0, 0, 1, 128, 0): ('bf16', 1, 1, 1, 192, 128, 0, 1, 0, 0, 0, (1, 128)),
    (1, 3, 0, 0, 0, 0, 1, 0, 256, 0): ('bf16', 0, 1, 1, 16, 64, 0, 0, 4, 0, 0, (1, 0)),
    (1, 3, 0, 0, 0, 0, 1, 1, 256, 0): ('bf16', 0, 1, 1, 1, 64, 0, 1, 0, 0, 0, (1, 0)),
    (1, 3, 0, 0, 0, 1, 1, 0, 256, 0): ('bf16', 0, 1, 1, 16, 64, 1, 0, 4, 0, 0, (1, 0)),
    (1, 3, 0, 0, 0, 1, 1, 1, 256, 0): ('bf16', 0, 1, 1, 1, 64, 1, 1, 0, 0, 0, (1, 0)),
    (1, 3, 0, 0, 1, 0, 1, 0, 256, 0): ('bf16', 0, 1, 1, 16, 64, 0, 0, 0, 0, 0, (1, 0)),
    (1, 3, 0, 0, 1, 1, 1, 0, 256, 0): ('bf16', 0, 1, 1, 16, 64, 1, 0, 0, 0, 0, (1, 0)),
    (1, 3, 0, 1, 0, 0, 1, 0, 256, 0): ('bf16', 0, 1, 1, 1, 64, 0, 0, 0, 0, 0, (1, 0)),
    (1, 3, 0, 1, 0, 1, 1, 0, 256, 0): ('bf16', 0, 1, 1, 1, 64, 1, 0, 0, 0, 0, (1, 0)),
    (1, 6, 0, 0, 0, 0, 1, 0, 256, 0): ('bf16', 0, 1, 1, 64, 64, 0, 0, 4, 0, 0, (1, 0)),
    (1, 6, 0, 0, 0, 0, 1, 1, 256, 0): ('bf16', 0, 1, 1, 64, 64, 0, 1, 0, 0, 0, (1, 0)),
    (1, 6, 0, 0, 0, 1, 1, 0, 256, 0): ('bf16', 0, 1, 1, 64, 64, 1, 0, 4, 0, 0, (1, 0)),
    (1, 6, 0, 0, 0, 1, 1, 1, 256, 0): ('bf16', 0, 1, 1, 64, 64, 1, 1, 0, 0, 0, (1, 0)),
    (1, 6, 0, 0, 1, 0, 1, 0, 256, 0): ('bf16', 0, 1, 1, 64, 64, 0, 0, 0, 0, 0, (1, 0)),
    (1, 6, 0, 0, 1, 1, 1, 0, 256, 0): ('bf16', 0, 1, 1, 64, 64, 1, 0, 0, 0, 0, (1, 0)),
    (1, 6, 0, 1, 0, 0, 1, 0, 256, 0): ('bf16', 1, 1, 1, 64, 64, 0, 0, 0, 0, 0, (1, 0)),
    (1, 8, 0, 0, 0, 0, 0, 0, 256, 0): ('bf16', 0, 1, 1, 127, 64, 0, 0, 4, 0, 0, (1, 0)),
    (1, 8, 0, 0, 0, 0, 1, 1, 256, 0): ('bf16', 0, 1, 1, 127, 64, 0, 1, 0, 0, 0, (1, 0)),
    (1, 8, 0, 0, 0, 1, 0, 0, 256, 0): ('bf16', 0, 1, 1, 127, 64, 1, 0, 4, 0, 0, (1, 0)),
    (1, 8, 0, 0, 0, 1, 1, 1, 256, 0): ('bf16', 0, 1, 1, 127, 64, 1, 1, 0, 0, 0, (1, 0)),
    (1, 8, 0, 0, 1, 0, 0, 0, 256, 0): ('bf16', 0, 1, 1, 128, 64, 0, 0, 0, 0, 0, (1, 0)),
    (1, 8, 0, 0, 1, 1, 0, 0, 256, 0): ('bf16', 0, 1, 1, 128, 64, 1, 0, 0, 0, 0, (1, 0)),
    (1, 8, 0, 1, 0, 0, 0, 0, 256, 0): ('bf16', 1, 1, 1, 127, 64, 0, 0, 0, 0, 0, (1, 0)),
    (1, 12, 0, 0, 0, 0, 0, 0, 256, 0): ('bf16', 0, 1, 1, 176, 64, 0, 0, 4, 0, 0, (1, 0)),
    (1, 12, 0, 0, 0, 0, 0, 1, 256, 0): ('bf16', 0, 1, 1, 176, 64, 0, 1, 0, 0, 0, (1, 0)),
    (1, 12, 0, 0, 0, 1, 0, 0, 256, 0): ('bf16', 0, 1, 1, 176, 64, 1, 0, 4, 0, 0, (1, 0)),
    (1, 12, 0, 0, 0, 1, 0, 1, 256, 0): ('bf16', 0, 1, 1, 176, 64, 1, 1, 0, 0, 0, (1, 0)),
    (1, 12, 0, 0, 1, 0, 0, 0, 256, 0): ('bf16', 0, 1, 1, 176, 64, 0, 0, 0, 0, 0, (1, 0)),
    (1, 12, 0, 0, 1, 1, 0, 0, 256, 0): ('bf16', 0, 1, 1, 176, 64, 1, 0, 0, 0, 0, (1, 0)),
    (1, 12, 0, 1, 0, 0, 0, 0, 256, 0): ('bf16', 1, 1, 1, 176, 64, 0, 0, 0, 0, 0, (1, 0)),
    (2, 0, 0, 0, 0, 0, 0, 0, 256, 0): ('bf16', 0, 1, 1, 127, 64, 0, 0, 0, 0, 0, (1, 0)),
    (3, 8, 1, 0, 0, 0, 0, 0, 256, 0): ('bf16', 0, 1, 1, 255, 64, 0, 0, 4, 0, 0, (1, 0)),
    (3, 8, 1, 0, 0, 0, 0, 1, 256, 0): ('bf16', 0, 1, 1, 255, 64, 0, 1, 0, 0, 0, (1, 0)),
    (3, 8, 1, 0, 1, 0, 0, 0, 256, 0): ('bf16', 0, 1, 1, 520, 64, 0, 0, 0, 0, 0, (1, 0)),
    (3, 8, 1, 1, 0, 0, 0, 0, 256, 0): ('bf16', 1, 1, 1, 255, 64, 0, 0, 0, 0, 0, (1, 0)),
    (3, 8, 2, 0, 0, 0, 0, 0, 256, 0): ('bf16', 0, 2, 510, 255, 16384, 0, 0, 4, 0, 0, (1, 0)),
    (3, 8, 2, 0, 0, 0, 0, 1, 256, 0): ('bf16', 0, 2, 510, 255, 16384, 0, 1, 0, 0, 0, (1, 0)),
    (3, 8, 2, 0, 1, 0, 0, 0, 256, 0): ('bf16', 0, 2, 510, 520, 16384, 0, 0, 0, 0, 0, (1, 0)),
    (3, 8, 2, 1, 0, 0, 0, 0, 256, 0): ('bf16', 1, 2, 510, 255, 16384, 0, 0, 0, 0, 0, (1, 0)),
    (3, 8, 3, 0, 0, 0, 0, 0, 256, 0): ('bf16', 0, 2, 765, 255, 16384, 0, 0, 4, 0, 0, (1, 0)),
    (3, 8, 3, 0, 0, 0, 0, 1, 256, 0): ('bf16', 0, 2, 765, 255, 16384, 0, 1, 0, 0, 0, (1, 0)),
    (3, 8, 3, 0, 1, 0, 0, 0, 256, 0): ('bf16', 0, 2, 765, 520, 16384, 0, 0, 0, 0, 0, (1, 0)),
    (3, 8, 3, 1, 0, 0, 0, 0, 256, 0): ('bf16', 1, 2, 765, 255, 16384, 0, 0, 0, 0, 0, (1, 0)),
    (4, 6, 0, 0, 0, 0, 0, 0, 128, 0): ('bf16', 0, 1, 1, 16, 1, 0, 0, 0, 0, 0, (1, 0)),
    (4, 6, 0, 1, 0, 0, 0, 0, 128, 0): ('bf16', 0, 1, 1, 1, 1, 0, 0, 0, 0, 0, (1, 0)),
    (4, 12, 0, 0, 0, 0, 0, 0, 128, 0): ('bf16', 0, 1, 1, 128, 1, 0, 0, 0, 0, 0, (1, 0)),
    (4, 12, 0, 1, 0, 0, 0, 0, 128, 0): ('bf16', 1, 1, 1, 127, 1, 0, 0, 0, 0, 0, (1, 0)),
    (5, 0, 0, 0, 0, 0, 0, 0, 128, 0): ('bf16', 0, 1, 1, 16, 1, 0, 0, 4, 0, 0, (1, 0)),
    (6, 0, 2, 0, 0, 0, 0, 0, 128, 0): ('f32', 0, 2, 765, 1, 16384, 0, 0, 0, 0, 0, (1, 0)),
    (6, 0, 2, 0, 0, 0, 0, 0, 128, 1): ('f32_split', 0, 2, 765, 1, 16384, 0, 0, 0, 0, 0, (1, 0)),
    (7, 0, 1, 0, 0, 0, 0, 0, 128, 0): ('f32', 0, 1, 1, 1, 64, 0, 0, 0, 0, 0, (1, 0)),
    (7, 0, 1, 0, 0, 0, 0, 0, 128, 1): ('f32_split', 0, 1, 1, 1, 64, 0, 0, 0, 0, 0, (1, 0)),
    (8, 0, 1, 0, 0, 0, 0, 0, 128, 0): ('f32', 0, 1, 1, 32, 64, 0, 0, 0, 0, 0, (1, 0)),
    (8, 0, 1, 0, 0, 0, 0, 0, 128, 1): ('f32_split', 0, 1, 1, 64, 64, 0, 0, 0, 0, 0, (1, 0)),
}


def run_case(case, seed=0, device="cuda:0", describe=True):
    """One call of ``SMALLEST`` through the public ops (``ops.pointwise.conv1x1_fwd`` / ``conv1x1_bwd``, with a
    ``PackedConv1x1Weights`` image where the case has one) under the case's ``oss_conv1x1_set_wg`` override.
    -> dict: ``got`` (y or dx), the operands ``x`` (the GEMM's activation operand: x or dy), ``w`` (cout, cin), ``bias``, ``res``,
    and ``describe`` = the ``oss_conv1x1_launch`` of the very pointers and strides the op handed to the library (None without)."""
    import ctypes

    import torch

    from vmambair_amd import _capi, _precision
    from vmambair_amd.ops import pointwise as pw

    io, dgrad, B, M, K, P, res, img, wa, xa, pad, ov = case
    dt = {"bf16": torch.bfloat16, "f16": torch.float16}.get(io, torch.float32)
    code = {"bf16": _capi.OSS_BF16, "f16": _capi.OSS_F16, "f32": _capi.OSS_F32, "f32_split": _capi.OSS_F32_BF16X3}[io]
    cout, cin = (K, M) if dgrad else (M, K)
    g = torch.Generator().manual_seed(seed)
    item = torch.empty(0, dtype=dt).element_size()
    assert wa % 4 == 0 and xa % item == 0

    def planes(channels):   # (B, channels, 1, P): channel stride P + pad, first element xa bytes behind a 16-byte boundary
        flat = torch.empty(B * channels * (P + pad) + 16, dtype=dt, device=device)
        t = flat[xa // item:].as_strided((B, channels, 1, P), (channels * (P + pad), P + pad, P, 1))
        t.copy_(torch.randn(B, channels, 1, P, generator=g).to(dt))
        return t

    a = planes(K)                                                 # forward: x (B, cin, P); input gradient: dy (B, cout, P)
    wflat = torch.empty(cout * cin + 4, device=device)
    w = wflat[wa // 4:wa // 4 + cout * cin].view(cout, cin, 1, 1)
    w.copy_((torch.randn(cout, cin, generator=g) * cin ** -0.5).view(cout, cin, 1, 1))
    bias = None if dgrad else torch.randn(cout, generator=g).to(device)
    r = torch.randn(B, cout, 1, P, generator=g).to(dt).to(device) if res else None
    lib = _capi.load()
    packed = None
    lib.oss_conv1x1_set_wg(*ov)
    try:
        if img:
            packed = pw.PackedConv1x1Weights([w], dt)
            packed.refresh()
            pw.set_packed_images(packed.images)
        with _precision.float32_matmul_precision("high" if io == "f32_split" else "highest"):
            if dgrad:
                x = torch.randn(B, cin, 1, P, generator=g).to(dt).to(device)
                got = pw.conv1x1_bwd(x, w, a, False)[0]
            else:
                got = pw.conv1x1_fwd(a, w, bias, r)
        o = None
        if describe:
            o = _capi._HDR.structs["oss_conv1x1_launch"]()
            image = packed.images[w.data_ptr()][3 + dgrad].data_ptr() if img else None
            rc = lib.oss_conv1x1_describe(dgrad, code, a.data_ptr(), w.data_ptr(), image, None if bias is None else bias.data_ptr(),
                                          None if r is None else r.data_ptr(), got.data_ptr(), B, cout, cin, P, a.stride(0), a.stride(1),
                                          ctypes.byref(o))
            assert rc == 0, rc
    finally:
        pw.clear_packed_images()
        lib.oss_conv1x1_set_wg(1, 0)
    return {"got": got, "x": a, "w": w.view(cout, cin), "bias": bias, "res": r, "describe": o, "dtype": dt}
