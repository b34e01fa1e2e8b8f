"""Every element of every EfficientNet-B0 gradient, at the shapes the backward had never run at.

The step is the one of ``test_b0_224_gpu.py`` (``b0_helpers.hip_step``: PretrainedBackboneDetector,
deterministic_init_, dropout 0, weighted CE with CLASS_W, ``b0_helpers.frames`` inputs).  The fp32 step
(exact fp32 MFMA) is held to the fp64 CPU oracle by the whole-tensor checker of ``b0_helpers.py``: per
tensor and per output channel, err <= K32 x max(torch-fp32's own error, floor), on every kernel path of
the ``kernel_paths`` fixture (default, forced, split_dw); logits, scores and loss at rtol 1e-3 /
atol 1e-5 and the BN running statistics at rtol 1e-4 / atol 1e-6 against the fp32 oracle.  bf16 and
fp16 (loss scale 1024) run at the same shapes on the default path under the existing per-tensor bound
``K_VS_AUTOCAST`` (``b0_helpers.vs_fp64``).

Cases, as (clips, frames per clip, H, W), each the smallest input that reaches the named launches.
``i.j`` is block j of stage i; the class of every depthwise backward launch below is what the plan's
launch-site log (``DFD_SITE_LOG``) recorded for the case, the tile follows from the dispatch code
(``dw_bwd1_covers`` / ``launch_dw_bwd1``, ``dw2_config``, ``launch_dw_bwd``, ``try_dw_fwd1``).
"generic" is ``launch_dw_bwd`` behind the BN2 apply pass on the default and forced paths and
``launch_dw_dgrad`` + ``launch_dw_wgrad`` on split_dw (where every layer below takes those two).

``w224`` (1, 2, 112, 224) -- the fast tiles at maps with H != W:
  0.0 k3 56x112: dw_bwd1<3,8,28> (7 x 4 tiles), forward dw_fwd1<3,8,28>;  1.0 k3 s2 from 56x112:
  dw_bwd2 8x56 (7 x 2);  1.1 k3 28x56: dw_bwd1<3,14,14> (2 x 4);  2.0 k5 s2 from 28x56: generic 8x8
  tiles (28 = 3.5 tiles: a tail row);  2.1 k5 14x28: dw_bwd1<5,14,14> (1 x 2);  3.0 k3 s2 from 14x28:
  generic;  3.1-3.2 k3 and 4.0-4.2 k5 at 7x14: generic 7x7 tiles, forward the generic tile kernel;
  5.0 k5 s2 from 7x14 and 5.1-5.3 k5, 6.0 k3 at 4x7: generic, partly empty 7x7 tiles.
``h224`` (1, 2, 224, 112) -- the transposed maps:
  0.0 112x56: dw_bwd1<3,8,28> two tiles wide (14 x 2), forward dw_fwd1<3,14,14>;  1.0 s2 from 112x56:
  dw_bwd2 8x56, a single tile column (14 x 1);  1.1 56x28: dw_bwd1<3,8,28> one tile wide (7 x 1);
  2.0 s2 from 56x28: generic;  2.1 28x14: dw_bwd1<5,14,14> (2 x 1);  3.0 s2 from 28x14: generic;
  14x7 and 7x4 maps: generic.
``t5`` (1, 5, 112, 112) -- an odd frame count on the stacked-frame tiles:
  0.0 56x56: dw_bwd1<3,8,28>;  1.0 s2 from 56x56: dw_bwd2 8x56;  1.1 28x28: dw_bwd1<3,14,14>;
  2.0 k5 s2 from 28x28: generic;  2.1 14x14: dw_bwd1<5,14,14>;  3.0 k3 s2 from 14x14: generic;
  3.1-3.2 k3 and 4.0-4.2 k5 at 7x7: dw_bwd1<.,7,7,7,2>, two frames per tile, the fifth frame alone in
  a half-empty tile (forward dw_fwd1<.,7,7,7,2> likewise);  5.0 k5 s2 from 7x7 and the 4x4 maps: generic.
``odd`` (1, 3, 100, 84) -- no map tiles: maps 50x42, 25x21, 13x11, 7x6, 4x3.  Every depthwise layer
  runs the generic forward and the generic backward (no dw_bwd1 / dw_bwd2 launch in the log); the
  stride-2 layers meet odd inputs (25x21 -> 13x11 -> 7x6: the last input row / column has no partner
  of the other parity), and the 1x1 GEMMs run at M = 3*50*42 = 6300, 3*25*21 = 1575, 3*13*11 = 429,
  3*7*6 = 126 and 3*4*3 = 36 rows, none a multiple of a GEMM tile.

Each case costs one fp64 oracle step on the CPU (1-2 s, cached for the module) and a fraction of a
second per HIP step.
"""
import pytest
import torch

import b0_helpers as bh

pytestmark = pytest.mark.gpu

SHAPES = {"w224": (1, 2, 112, 224), "h224": (1, 2, 224, 112), "t5": (1, 5, 112, 112), "odd": (1, 3, 100, 84)}


@pytest.mark.parametrize("case", list(SHAPES))
def test_grad_full_fp32(cuda, case, kernel_paths):
    shape = SHAPES[case]
    ref = bh.oracle_step(shape)
    logits, scores, loss, grads, bufs = bh.hip_step(shape, "fp32", cuda)
    torch.testing.assert_close(logits, ref["logits"], rtol=1e-3, atol=1e-5)
    torch.testing.assert_close(scores, ref["scores"], rtol=1e-3, atol=1e-5)
    assert abs(loss - ref["loss"]) <= 1e-3 * abs(ref["loss"]) + 1e-5
    for n, rb in ref["bufs"].items():
        torch.testing.assert_close(bufs[n], rb, rtol=1e-4, atol=1e-6, msg=lambda m: f"{n}: {m}")
    bh.check_grads_full(grads, shape, f" {case}/{kernel_paths}")


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", list(SHAPES))
def test_grad_full_16bit(cuda, case, dtype):
    shape = SHAPES[case]
    ref = bh.oracle_step(shape)
    logits, _, loss, grads, bufs = bh.hip_step(shape, dtype, cuda,
                                               loss_scale=bh.FP16_LOSS_SCALE if dtype == "fp16" else 1.0)
    torch.testing.assert_close(logits, ref["logits"], rtol=5e-2, atol=5e-2)
    assert all(torch.isfinite(g).all() for g in grads.values())
    bh.vs_fp64(shape, dtype, loss, grads, f" {case}")
    # BN running statistics, anchored like the gradients: relative L2 distance to the fp32 oracle within
    # K_VS_AUTOCAST x torch-bf16-autocast's own distance on that buffer (floor AUTOCAST_FLOOR).  (At 2-5
    # frames the 7x4 / 4x4 maps give a BN 32-80 samples per channel: single late-stage variances move by
    # 3 % under bf16 storage, in torch's autocast as in the HIP step.)
    ac = bh.autocast_buf_err(shape)
    rows = sorted(((bh.rel_err(bufs[n], rb) / max(ac[n], bh.AUTOCAST_FLOOR), n) for n, rb in ref["bufs"].items()),
                  reverse=True)
    print(f"{case} {dtype}: worst running-stat err / autocast err: " + "; ".join(f"{n} {q:.3f}" for q, n in rows[:4]))
    assert rows[0][0] <= bh.K_VS_AUTOCAST[dtype], rows[:4]
