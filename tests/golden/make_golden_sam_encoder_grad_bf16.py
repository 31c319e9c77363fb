"""Writes tests/golden/sam_encoder_grad_bf16.npz: the yardstick of the encoder's bf16 TRAINING mode -- how far the parameter
gradients of the reference's layers/backbones/sam_encoder.py move, for the fixture model of sam_encoder.npz, when it runs under
bf16 autocast with autograd instead of in float64.

The reference module is imported unmodified (as make_golden_sam_encoder.py does), loaded with the weights and the input of
tests/golden/sam_encoder.npz, and differentiated under ``torch.autocast('cpu', dtype=torch.bfloat16)`` -- the mode the reference's
Lightning harness trains in (``--amp_backend native``) -- with the upstream gradients ``cot`` of sam_encoder_grad.npz (the
``forward`` output) and sam_encoder_grad_embed.npz (the neck output).  The float64 gradients are the ones those fixtures hold.

Stored, scalars only, per run (``forward`` / ``embed``) and parameter:
    <run>/max_abs/<name>    max |autocast gradient - float64 gradient|
    <run>/rel_l2/<name>     || autocast gradient - float64 gradient || / || float64 gradient ||
The model test (tests/test_vit_grad_bf16_gpu.py) holds every gradient of the bf16 training mode to
max(2 x the stored error, 2^-21 max |gradient|) in both measures (the relative floor 2^-21 as it stands).

Asserted here: each of the four misreadings of make_golden_sam_encoder_grad.py (padding gradients left out of qkv.bias, rel-pos
terms left out of dq, a scaled q in dRh / dRw, padding slots as queries) moves its named gradient, under the ``forward`` upstream
gradient, by more than 3 x that gradient's model bar in the max-abs measure.

    python tests/golden/make_golden_sam_encoder_grad_bf16.py /path/to/reference
"""
import os
import sys
from functools import partial

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import vit_grad_ref as VG                                  # noqa: E402
import vit_ref as V                                        # noqa: E402
from make_golden_sam_encoder import import_reference       # noqa: E402
from make_golden_sam_encoder_grad import MISREADINGS       # noqa: E402

MARGIN = 2.0


def model_bar(err, grad):
    return max(MARGIN * float(err), 2.0 ** -21 * float(grad.abs().max()))


def autocast_grads(model, img, cot, embed):
    model.zero_grad()
    kept = []
    hook = model.neck.register_forward_hook(lambda m, i, o: kept.append(o))
    with torch.autocast('cpu', dtype=torch.bfloat16):
        out = model(img)
        hook.remove()
        if embed:
            out = kept[0].permute(0, 2, 3, 1)
        loss = (out.float() * cot).sum()
    loss.backward()
    return {k: p.grad.detach().double() for k, p in model.named_parameters()}


def main(root):
    ref = import_reference(root)
    cfg = V.FIXTURE_CFG
    base = np.load(os.path.join(HERE, 'sam_encoder.npz'))
    wts = {k[2:]: torch.from_numpy(base[k]) for k in base.files if k.startswith('w/')}
    img = torch.from_numpy(base['input'])
    model = ref.ImageEncoderViT(
        img_size=cfg['img_size'], patch_size=cfg['patch_size'], embed_dim=cfg['embed_dim'], depth=cfg['depth'],
        num_heads=cfg['num_heads'], out_chans=cfg['out_chans'], window_size=cfg['window_size'],
        global_attn_indexes=cfg['global_attn_indexes'], use_rel_pos=True, norm_layer=partial(torch.nn.LayerNorm, eps=cfg['eps']),
        final_dim=cfg['final_dim'], downsample_factor=cfg['downsample_factor']).eval().float()
    model.load_state_dict(wts)

    data, report = {}, {}
    for embed in (False, True):
        run = 'embed' if embed else 'forward'
        fx = VG.open_fixture(HERE, embed)
        cot = torch.from_numpy(fx['cot'])
        got = autocast_grads(model, img.float(), cot, embed)
        errs = {}
        for k, g in got.items():
            want = VG.fixture_grad(fx, k)
            assert bool(torch.isfinite(g).all()) and g.shape == want.shape, k
            errs[k] = float((g - want).abs().max())
            data[f'{run}/max_abs/{k}'] = np.float64(errs[k])
            data[f'{run}/rel_l2/{k}'] = np.float64(float((g - want).norm() / want.norm()))
        rel = sorted(float(data[f'{run}/rel_l2/{k}']) for k in got)
        report[run] = dict(parameters=len(got), median_rel_l2=rel[len(rel) // 2], worst_rel_l2=rel[-1], best_rel_l2=rel[0],
                           worst=max(got, key=lambda k: float(data[f'{run}/rel_l2/{k}'])))
        if not embed:
            for label, kw, name in MISREADINGS:
                want = VG.fixture_grad(fx, name)
                wrong = VG.encoder_backward(wts, cfg, img.double(), cot.double(), embed=False, **kw)
                moved = float((wrong[name] - want).abs().max())
                b = model_bar(errs[name], want)
                assert moved > 3.0 * b, (label, name, moved, b)
                report[label] = round(moved / b, 1)
    path = os.path.join(HERE, 'sam_encoder_grad_bf16.npz')
    np.savez_compressed(path, **data)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1000000
    print(report)


if __name__ == '__main__':
    main(sys.argv[1])
