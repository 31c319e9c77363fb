"""GPU: SAM's prompt encoder and mask decoder (sgv3d_amd.segment_anything, csrc/sam_decoder.hip, sgv3d_amd/sam_masks.py).

  attention    sgv3d_sam_attention against float64 under the a-priori bar of DESIGN.md section 21 without the rel-pos terms;
               bit-level known answers; edge inputs; guard bands; repeat launches
  decoder      low-res logits and IoU predictions against tests/sam_ref.py in float64: at most 4 x the error of the restatement's
               own float32 CPU run on the same inputs
  known        answers that do not depend on the restatement
  compose      sgv3d_sam_mask_compose against its host twin, bit for bit
  whole path   SamPredictor on a two-block encoder, get_sam_mask into FrameRecombiner.combine, graph replay, reloaded weights

Measured ratios (device error / float32 CPU error of the restatement, MI355X): see DESIGN.md section 25.
"""
import math
import os
import sys
from functools import partial

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import sam_masks_cases as C          # noqa: E402
import sam_ref                       # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U32 = 2.0 ** -24


def _ops():
    from sgv3d_amd.segment_anything import ops
    return ops


# ---------------------------------------------------------------------------------------------------------------- attention
def _attn_ref(q, k, v, heads):
    b, nq, c = q.shape
    hd = c // heads
    sp = lambda t: t.double().reshape(b, -1, heads, hd).transpose(1, 2)
    qq, kk, vv = sp(q), sp(k), sp(v)
    a = torch.softmax(qq @ kk.transpose(-1, -2) / math.sqrt(hd), -1) @ vv
    return a.transpose(1, 2).reshape(b, nq, c)


def _attn_bar(q, k, v, heads):
    """|out - ref| bound per (query, channel), from the inputs only (rel-pos terms dropped)."""
    b, nq, c = q.shape
    hd, T = c // heads, k.shape[1]
    sp = lambda t: t.double().reshape(b, -1, heads, hd).transpose(1, 2)
    qq, kk, vv = sp(q), sp(k), sp(v)
    E = ((hd + 3) * U32 * (qq.abs() @ kk.abs().transpose(-1, -2)) / math.sqrt(hd)).amax(-1, keepdim=True)      # [b, h, nq, 1]
    spread = (vv.amax(2, keepdim=True) - vv.amin(2, keepdim=True))                                              # [b, h, 1, hd]
    bar = 2 * ((2 * E + 8 * U32) * spread + (T + 8) * U32 * vv.abs().amax(2, keepdim=True))
    return bar.transpose(1, 2).reshape(b, nq, c)


@pytest.mark.parametrize("nq,nk,hd,batch", C.ATTENTION_SHAPES)
def test_attention_against_float64(nq, nk, hd, batch):
    heads = 8 if hd == 16 else 4
    g = torch.Generator().manual_seed(nq * 100003 + nk * 17 + hd)
    q, k, v = (torch.randn(batch, n, heads * hd, generator=g) * s for n, s in ((nq, 1.5), (nk, 1.5), (nk, 1.0)))
    out = _ops().sam_attention(q.to(DEV), k.to(DEV), v.to(DEV), heads).cpu()
    ref, bar = _attn_ref(q, k, v, heads), _attn_bar(q, k, v, heads)
    ratio = ((out.double() - ref).abs() / bar).max().item()
    print(f"attention nq {nq} nk {nk} hd {hd}: worst error / bar {ratio:.4f}")
    assert torch.isfinite(out).all() and ratio <= 1.0


@pytest.mark.parametrize("nq,nk", [(7, 600), (7, 36), (300, 7)])
def test_attention_known_answers_bit_for_bit(nq, nk):
    ops, heads, hd = _ops(), 8, 16
    g = torch.Generator().manual_seed(5)
    # a dominant key: its logit is 600 above every other, the others' weights are exactly zero
    v = torch.randn(1, nk, heads * hd, generator=g)
    q = torch.ones(1, nq, heads * hd)
    k = torch.full((1, nk, heads * hd), -75.0 / 4)         # logit 16 * (-18.75) / 4 = -75 ... times q = 1
    star = nk - 3
    k[0, star] = 75.0 / 4 * 7
    out = ops.sam_attention(q.to(DEV), k.to(DEV), v.to(DEV), heads).cpu()
    assert torch.equal(out, v[:, star:star + 1].expand(1, nq, -1))
    # uniform weights: q = 0 gives every key the weight 1 / nk; integer values make the sum exact
    vi = torch.randint(-8, 9, (1, nk, heads * hd), generator=g).float()
    out = ops.sam_attention(torch.zeros(1, nq, heads * hd, device=DEV), torch.randn(1, nk, heads * hd, generator=g).to(DEV), vi.to(DEV), heads).cpu()
    assert torch.equal(out, (vi.sum(1, keepdim=True) / nk).expand(1, nq, -1))


def test_attention_edge_inputs_guard_bands_and_repeats():
    ops, heads, hd = _ops(), 8, 16
    c = heads * hd
    g = torch.Generator().manual_seed(9)
    for nq, nk in ((7, 300), (260, 7)):
        q, k, v = torch.randn(2, nq, c, generator=g), torch.randn(2, nk, c, generator=g), torch.randn(2, nk, c, generator=g)
        # logits of +-300 in head 0, all logits <= -50 in head 1
        q[:, :, :hd] = 5.0
        k[:, :, :hd] = torch.where(torch.rand(2, nk, 1, generator=g) < 0.5, 15.0, -15.0).expand(-1, -1, hd)
        q[:, :, hd:2 * hd] = 4.0
        k[:, :, hd:2 * hd] = -(3.2 + torch.rand(2, nk, hd, generator=g))
        # row-strided operands inside wider buffers whose other columns are NaN (guard bands), NaN pre-filled output
        wide = lambda t: torch.full((t.shape[0], t.shape[1], c + 8), float("nan")).to(DEV)
        qw, kw, vw, ow = wide(q), wide(k), wide(v), wide(q)
        qw[..., 4:4 + c], kw[..., :c], vw[..., 8:], = q.to(DEV), k.to(DEV), v.to(DEV)
        out = ops.sam_attention(qw[..., 4:4 + c], kw[..., :c], vw[..., 8:], heads, out=ow[..., 4:4 + c])
        got = ow.cpu()
        assert torch.isnan(got[..., :4]).all() and torch.isnan(got[..., 4 + c:]).all(), "the guard bands were written"
        res = got[..., 4:4 + c]
        ref, bar = _attn_ref(q, k, v, heads), _attn_bar(q, k, v, heads)
        assert torch.isfinite(res).all() and ((res.double() - ref).abs() <= bar).all()
        again = ops.sam_attention(q.to(DEV), k.to(DEV), v.to(DEV), heads)
        assert torch.equal(again.cpu(), res) and torch.equal(ops.sam_attention(q.to(DEV), k.to(DEV), v.to(DEV), heads), again)
        assert out.data_ptr() == ow[..., 4:4 + c].data_ptr()


# ------------------------------------------------------------------------------------------------------------------ decoder
def _product_from(ref_model, grid, img_size, with_encoder=False):
    from sgv3d_amd.layers.backbones.sam_encoder import ImageEncoderViT
    from sgv3d_amd.segment_anything.modeling import MaskDecoder, PromptEncoder, Sam, TwoWayTransformer
    enc = ImageEncoderViT(img_size=img_size, patch_size=16, embed_dim=64, depth=2 if with_encoder else 0, num_heads=2, out_chans=256,
                          use_rel_pos=True, window_size=4, global_attn_indexes=(1,), norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    sam = Sam(enc, PromptEncoder(256, (grid, grid), (img_size, img_size), 16),
              MaskDecoder(transformer_dim=256, transformer=TwoWayTransformer(2, 256, 8, 2048)))
    sd = ref_model.state_dict()
    if not with_encoder:
        sd = dict(sd, **{"image_encoder." + k: v for k, v in enc.state_dict().items()})
    sam.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    return sam.to(DEV).eval()


def _decoder_case(case):
    ref64, emb, boxes, frames = C.decoder_case(case)
    low64, iou64 = C.run_ref(ref64, emb, boxes, frames, torch.float64, case.multimask)
    low32, iou32 = C.run_ref(ref64, emb, boxes, frames, torch.float32, case.multimask)
    return ref64, emb, boxes, frames, (low64, iou64), (low32, iou32)


@pytest.mark.parametrize("case", C.DECODER_CASES, ids=lambda c: c.name)
def test_decoder_against_the_float64_restatement(case):
    ref64, emb, boxes, frames, (low64, iou64), (low32, iou32) = _decoder_case(case)
    sam = _product_from(ref64, case.grid, 16 * case.grid)
    fob = torch.tensor(frames, dtype=torch.int32, device=DEV)
    tokens = sam.prompt_encoder.box_tokens(boxes.float().to(DEV), sam.mask_decoder.iou_token.weight, sam.mask_decoder.mask_tokens.weight)
    low, iou = sam.mask_decoder(emb.float().to(DEV).contiguous(), fob, sam.prompt_encoder.get_dense_pe_nhwc(), tokens,
                                sam.prompt_encoder.no_mask_embed.weight, case.multimask)
    low, iou = low.cpu().double(), iou.cpu().double()
    assert low.shape == low64.shape and iou.shape == iou64.shape
    e_low, e_iou = (low - low64).abs().max().item(), (iou - iou64).abs().max().item()
    b_low, b_iou = (low32.double() - low64).abs().max().item(), (iou32.double() - iou64).abs().max().item()
    print(f"decoder {case.name}: low-res error {e_low:.3e} (float32 CPU {b_low:.3e}, ratio {e_low / b_low:.2f}); "
          f"iou error {e_iou:.3e} (float32 CPU {b_iou:.3e}, ratio {e_iou / b_iou:.2f})")
    assert e_low <= 4 * b_low and e_iou <= 4 * b_iou
    # masks: a pixel may differ from the float64 restatement only where its float64 logit is within the same bar of zero
    hw, size = case.original, 16 * case.grid
    pre = sam_ref.get_preprocess_shape(hw[0], hw[1], size)
    out64 = sam_ref.postprocess_masks(low64, size, pre, hw)
    b, n = low.shape[:2]
    got = _ops().mask_compose(_ops().COMPOSE_BOOL, low.float().reshape(b * n, *low.shape[2:]).to(DEV).contiguous(), size, pre, hw).cpu()
    differ = got.reshape(out64.shape) != (out64 > 0)
    excused = out64.abs() <= 4 * b_low
    assert not (differ & ~excused).any()
    assert excused.float().mean().item() <= 0.005


def test_zero_q_proj_gives_out_proj_of_the_mean_of_v():
    from sgv3d_amd.segment_anything.modeling import Attention
    torch.manual_seed(3)
    att = Attention(256, 8, downsample_rate=2).to(DEV)
    with torch.no_grad():
        att.q_proj.weight.zero_()
        att.q_proj.bias.zero_()
    q, kv = torch.randn(2, 1, 7, 256, device=DEV), torch.randn(2, 5, 8, 256, device=DEV)
    out = att(q, kv, kv).cpu().double()
    v = kv.cpu().double().reshape(2, 40, 256) @ att.v_proj.weight.cpu().double().t() + att.v_proj.bias.cpu().double()
    want = v.mean(1, keepdim=True) @ att.out_proj.weight.cpu().double().t() + att.out_proj.bias.cpu().double()
    assert (out.reshape(2, 7, 256) - want).abs().max().item() < 2e-5


def test_a_rectangle_of_plus_one_goes_through_compose():
    ops = _ops()
    low, size = 24, 96
    logit = -torch.ones(1, low, low)
    logit[0, 4:10, 6:16] = 1.0
    for hw in ((54, 96), (27, 48), (135, 240)):
        pre = sam_ref.get_preprocess_shape(hw[0], hw[1], size)
        got = ops.mask_compose(ops.COMPOSE_BOOL, logit.to(DEV), size, pre, hw).cpu()[0]
        val = ops.mask_compose(ops.COMPOSE_LOGIT, logit.to(DEV), size, pre, hw).cpu()[0]
        assert val.min() >= -1 and val.max() <= 1 and torch.equal(got, val > 0)
        # the map is -1 + 2 a(y) b(x) with a, b the 0 .. 1 ramps between neighbouring low-res centres: the rectangle's edges sit where
        # a or b crosses 1/2, at 16 .. 40 x 24 .. 64 of the square (low-res rows 4 .. 9, columns 6 .. 15, four pixels a cell), times
        # original / preprocess in the frame; one pixel of the square inside them a, b >= 3/4 and a b > 1/2 also at the corners.  The
        # second resize mixes neighbours one frame pixel apart.
        ry, rx = hw[0] / pre[0], hw[1] / pre[1]
        my, mx = ry + 1, rx + 1
        ys, xs = (torch.arange(hw[0]) + 0.5), (torch.arange(hw[1]) + 0.5)
        inside = ((ys > 16 * ry + my) & (ys < 40 * ry - my))[:, None] & ((xs > 24 * rx + mx) & (xs < 64 * rx - mx))[None, :]
        outside = ((ys < 16 * ry - my) | (ys > 40 * ry + my))[:, None] | ((xs < 24 * rx - mx) | (xs > 64 * rx + mx))[None, :]
        assert got[inside].all() and not got[outside].any() and inside.any() and outside.any()


# ------------------------------------------------------------------------------------------------------------------ compose
@pytest.mark.parametrize("hw", C.COMPOSE_SIZES)
def test_compose_is_the_host_twin_bit_for_bit(hw):
    ops = _ops()
    size, low = 96, 24
    pre = sam_ref.get_preprocess_shape(hw[0], hw[1], size)
    logits, labels, frames, n_frames = C.compose_case(hw, low)
    dl = torch.from_numpy(logits).to(DEV)
    lab, fob = torch.tensor(labels, dtype=torch.int32, device=DEV), torch.tensor(frames, dtype=torch.int32, device=DEV)
    got = ops.mask_compose(ops.COMPOSE_CLASS, dl, size, pre, hw, lab, fob, n_frames).cpu().numpy()
    want = ops.mask_compose_host(ops.COMPOSE_CLASS, logits, size, pre, hw, labels, frames, n_frames)
    assert np.array_equal(got, want)
    assert got[1].max() == 0, "the empty frame"
    assert got.max() == 6 and set(np.unique(got)) >= {0, 2, 6}
    for mode in (ops.COMPOSE_BOOL, ops.COMPOSE_LOGIT):
        g = ops.mask_compose(mode, dl, size, pre, hw).cpu().numpy()
        assert np.array_equal(g, ops.mask_compose_host(mode, logits, size, pre, hw))
    # the paint loop over the per-box masks is the class image
    masks = ops.mask_compose_host(ops.COMPOSE_BOOL, logits, size, pre, hw)
    for f in range(n_frames):
        sel = [i for i, fr in enumerate(frames) if fr == f]
        assert np.array_equal(sam_ref.paint([masks[i] for i in sel], [labels[i] for i in sel], hw), want[f])
    # a box on the last row and column reaches the last pixel
    assert want[2][-1, -1] == 3


# --------------------------------------------------------------------------------------------------------------- whole path
@pytest.fixture(scope="module")
def whole():
    ref64 = sam_ref.randomize_(sam_ref.build(), C.WHOLE_SEED).double()
    sam = _product_from(ref64, 6, 96, with_encoder=True)
    return ref64, sam


def test_pillow_bilinear_resize_bit_for_bit():
    z = np.load(os.path.join(HERE, "golden", "sam_masks.npz"))
    ops = _ops()
    for key in [k for k in z.files if k.startswith("resize_src_")]:
        tag = key[len("resize_src_"):]
        src, want = z[key], z["resize_out_" + tag]
        got = ops.resize_bilinear_u8(torch.from_numpy(src).to(DEV).unsqueeze(0), want.shape[:2])[0].cpu().numpy()
        assert np.array_equal(got.transpose(1, 2, 0), want.astype(np.float32)), tag


def test_predictor_against_the_restatement_and_strict_state_dicts(whole):
    from sgv3d_amd.segment_anything import SamPredictor
    ref64, sam = whole
    assert not ref64.load_state_dict({k: v.double() for k, v in sam.state_dict().items()}, strict=True).missing_keys
    pred = SamPredictor(sam)
    frame, boxes = C.whole_frame()
    hw = frame.shape[:2]
    pred.set_image(torch.from_numpy(frame).to(DEV))
    tb = pred.transform.apply_boxes_torch(torch.tensor(boxes), hw)
    assert torch.equal(tb, sam_ref.apply_boxes(torch.tensor(boxes), hw, 96))
    masks, iou, low = pred.predict_torch(None, None, boxes=tb.to(DEV), multimask_output=False)
    assert masks.shape == (len(boxes), 1, *hw) and masks.dtype == torch.bool and low.shape == (len(boxes), 1, 24, 24) and iou.shape == (len(boxes), 1)
    low64, iou64, low32, iou32, out64 = C.whole_reference(ref64, frame, boxes)
    e, b = (low.cpu().double() - low64).abs().max().item(), (low32.double() - low64).abs().max().item()
    ei, bi = (iou.cpu().double() - iou64).abs().max().item(), (iou32.double() - iou64).abs().max().item()
    print(f"whole path: low-res error {e:.3e} (float32 CPU {b:.3e}, ratio {e / b:.2f}); iou {ei:.3e} ({bi:.3e}, ratio {ei / bi:.2f})")
    assert e <= 4 * b and ei <= 4 * bi
    differ = masks.cpu() != (out64 > 0)
    excused = out64.abs() <= 4 * b
    assert not (differ & ~excused).any() and excused.float().mean().item() <= 0.005
    logits = pred.predict_torch(None, None, boxes=tb.to(DEV), multimask_output=False, return_logits=True)[0]
    assert (logits.cpu().double() - out64).abs().max().item() <= 4 * b + 1e-6
    multi = pred.predict_torch(None, None, boxes=tb.to(DEV), multimask_output=True)
    assert multi[0].shape == (len(boxes), 3, *hw) and multi[1].shape == (len(boxes), 3)
    with pytest.raises(NotImplementedError, match="point_coords"):
        pred.predict_torch(torch.zeros(1, 1, 2, device=DEV), None, boxes=tb.to(DEV))
    with pytest.raises(NotImplementedError, match="mask_input"):
        pred.predict_torch(None, None, boxes=tb.to(DEV), mask_input=torch.zeros(1, 1, 24, 24, device=DEV))


def test_get_sam_mask_feeds_the_recombiner_and_replays_in_a_graph(whole):
    import recombine_util as U
    from sgv3d_amd import recombine as RC, sam_masks
    from sgv3d_amd.segment_anything import SamPredictor
    ref64, sam = whole
    pred = SamPredictor(sam)
    h, w = 54, 96
    dest, sources = U.make_scene(51, h, w, n_dest_obj=2, n_src_obj=4)
    frames = [dest] + sources
    stack = torch.from_numpy(np.stack([f['image'] for f in frames])).to(DEV)
    boxes = [np.array([[5, 4, 60, 40], [30, 10, 90, 50], [0, 0, 95, 53]])[: 1 + i % 3] for i in range(len(frames))]
    labels = [[6, 9, 2][: 1 + i % 3] for i in range(len(frames))]
    batch = sam_masks.mask_images(pred, stack, boxes, labels)
    assert batch.shape == (len(frames), h, w) and batch.dtype == torch.uint8 and batch.is_cuda and int(batch.max()) <= 6
    single = sam_masks.get_sam_mask(pred, torch.tensor(boxes[2]), labels[2], stack[2])
    assert torch.equal(single, batch[2])
    assert int(sam_masks.get_sam_mask(pred, torch.zeros(0, 4), [], stack[0]).max()) == 0
    assert int(sam_masks.get_sam_mask(pred, torch.tensor([[0, 0, 0, 0]]), [0], stack[0]).max()) == 0
    # into FrameRecombiner.combine: the same result as the host entry fed the same masks
    host_frames = [dict(f, mask=batch[i].cpu().numpy()) for i, f in enumerate(frames)]
    dev_frames = [dict(f, image=stack[i], mask=batch[i]) for i, f in enumerate(frames)]
    res = RC.FrameRecombiner(src_hw=(h, w), max_obj=32).combine([dev_frames[0]], [dev_frames[1:]])
    host = U.host_entry([(host_frames[0], host_frames[1:])], max_obj=32, want_warped=False)
    assert np.array_equal(res.masks.cpu().numpy(), host['masks']) and np.array_equal(res.frames.cpu().numpy(), host['images'])
    # graph replay of the decoder + compose on a set image, bit for bit, also after the inputs changed in place
    pred.set_images(stack[:2])
    tb = pred.transform.apply_boxes_torch(torch.tensor(np.concatenate(boxes[:2])), (h, w)).to(DEV)
    lab = torch.tensor(labels[0] + labels[1], dtype=torch.int32, device=DEV)
    fob = torch.tensor([0] * len(labels[0]) + [1] * len(labels[1]), dtype=torch.int32, device=DEV)
    eager = pred.class_masks(tb, lab, fob).clone()
    assert torch.equal(eager, batch[:2])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = pred.class_masks(tb, lab, fob)
    captured.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager)
    # reloaded weights are seen: the caches follow the parameter versions
    other = sam_ref.randomize_(sam_ref.build(), C.WHOLE_SEED + 1)
    sam.load_state_dict({k: v.float() for k, v in other.state_dict().items()}, strict=True)
    pred.set_images(stack[:2])
    moved = pred.class_masks(tb, lab, fob)
    low64 = C.run_ref(other.double(), other.double().image_encoder(C.preprocessed(np.stack([f['image'] for f in frames[:2]]), 96)),
                      tb.cpu().double(), fob.tolist(), torch.float64, False)[0]
    pre = sam_ref.get_preprocess_shape(h, w, 96)
    out64 = sam_ref.postprocess_masks(low64, 96, pre, (h, w))[:, 0]
    want = np.stack([sam_ref.paint([(out64[i] > 0).numpy() for i in range(len(fob)) if fob[i] == f],
                                   [int(lab[i]) for i in range(len(fob)) if fob[i] == f], (h, w)) for f in range(2)])
    near = (out64.abs() <= 1e-4).any(0).numpy()
    assert not torch.equal(moved, eager) and np.array_equal(np.where(near, 0, moved.cpu().numpy()), np.where(near, 0, want))
    sam.load_state_dict({k: v.float() for k, v in ref64.state_dict().items()}, strict=True)


def test_rejections_before_any_launch(whole):
    from sgv3d_amd import _lib, sam_masks
    from sgv3d_amd.segment_anything import SamPredictor
    from sgv3d_amd.segment_anything.modeling import TwoWayTransformer
    ref64, sam = whole
    pred = SamPredictor(sam)
    with pytest.raises(_lib.SGV3DError, match="on the GPU"):
        pred.set_torch_image(torch.zeros(1, 3, 54, 96), (54, 96))
    with pytest.raises(_lib.SGV3DError, match="on the GPU"):
        sam_masks.get_sam_mask(pred, torch.zeros(1, 4), [1], torch.zeros(54, 96, 3, dtype=torch.uint8))
    pred.set_image(torch.zeros(54, 96, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(_lib.SGV3DError, match="on the GPU"):
        pred.predict_torch(None, None, boxes=torch.zeros(1, 4))
    with pytest.raises(_lib.SGV3DError, match="requires grad"):
        pred.predict_torch(None, None, boxes=torch.zeros(1, 4, device=DEV, requires_grad=True))
    with pytest.raises(_lib.SGV3DError, match=r"frame_index must hold one index in \[0, 1\)"):
        pred.predict_torch(None, None, boxes=torch.zeros(1, 4, device=DEV), frame_index=[1])
    t = TwoWayTransformer(1, 128, 2, 64).to(DEV)
    with pytest.raises(_lib.SGV3DError, match="not covered"):
        t(torch.zeros(1, 2, 2, 128, device=DEV), torch.zeros(1, 2, 2, 128, device=DEV), torch.zeros(1, 1, 7, 128, device=DEV))
