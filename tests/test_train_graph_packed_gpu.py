"""``GraphedTrainStep(packed_weights=True)`` -- the MFMA 1x1 convolutions on pre-packed 16-bit weight images, repacked by one
captured launch at the head of every step -- against ``packed_weights=False`` (the same kernels narrowing the fp32 masters in
their loaders).

Which comparison holds: the replayed step is run-to-run bit-stable (fixed-order partial sums everywhere, no floating-point
atomics) and the packed kernels add the same products in the same order, so the two sides are compared with ``torch.equal`` --
loss of every step, every parameter, every EMA tensor.

Four steps, not one: steps 2 - 4 are only equal if every replay repacks from the weights the fused optimizer has just written
through its raw pointers (the liveness of the images).  An image that stayed at its capture-time content would first show in
step 2's loss.
"""
import pytest
import torch

from vmambair_amd import ops

pytestmark = [pytest.mark.gpu, pytest.mark.selfcheck]
DEV = "cuda:0"


def _run(packed: bool, micro: int, steps: int):
    from vmambair_amd.archs import MambaSISR6
    from vmambair_amd.train_graph import GraphedTrainStep
    torch.manual_seed(0)
    net = MambaSISR6(dim=48, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1).to(DEV)
    torch.manual_seed(5)
    lq = torch.rand(2, 3, 32, 32, device=DEV)
    gt = torch.rand(2, 3, 128, 128, device=DEV)
    step = GraphedTrainStep(net, autocast_dtype=torch.bfloat16, warmup=1, micro_streams=micro, packed_weights=packed)
    assert (step.packed is not None) == packed
    if packed:
        # in_conv, out_conv, project_in, project_out of every block + the two reduce_chan layers of the decoder
        assert len(step.packed.images) >= 4 * 7 and not any(n.rsplit(".", 2)[-2] in ("in_conv", "project_out") for n in step.shadow)
    losses = [step(lq, gt).clone() for _ in range(steps)]
    torch.cuda.synchronize()
    assert ops.pointwise.packed_images_active() == 0, "the registry must be empty outside a step"
    return losses, [p.detach().clone() for p in net.parameters()], [e.clone() for e in step.ema]


@pytest.mark.parametrize("micro,steps", [(1, 4), (2, 2)], ids=["one_branch_4_steps", "two_branches_2_steps"])
def test_packed_weights_step_is_bit_identical_to_the_fp32_weight_step(micro, steps):
    got = _run(True, micro, steps)
    want = _run(False, micro, steps)
    for i, (a, b) in enumerate(zip(got[0], want[0])):
        assert torch.equal(a, b), f"loss of step {i + 1}: {float(a)!r} vs {float(b)!r}"
    assert float(got[0][-1]) != float(got[0][0]), "the weights moved"
    for what, g, w in (("parameter", got[1], want[1]), ("ema", got[2], want[2])):
        assert len(g) == len(w)
        for k, (a, b) in enumerate(zip(g, w)):
            assert torch.equal(a, b), f"{what} {k}: max |diff| {float((a - b).abs().max()):.3e}"
