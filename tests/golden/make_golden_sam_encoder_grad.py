"""Writes tests/golden/sam_encoder_grad.npz, sam_encoder_grad_embed.npz and their remainder files: the parameter gradients that the reference's layers/backbones/sam_encoder.py gives
under torch autograd for the model, weights and input of tests/golden/sam_encoder.npz (tests/vit_ref.py's FIXTURE_CFG: a window-5
block on a 12 x 12 map that pads to 15 x 15 and a global block, rel-pos on, a non-zero qkv bias).

The reference module is imported unmodified, with the ``cv2`` stub of make_golden_sam_encoder.py.  Two seeded cotangents are drawn
and stored as float32: ``cot`` [2, 32, 13, 24] for ``forward`` and ``cot_embed`` [2, 12, 12, 32] (NHWC) for the neck output that
``ImageEncoderViT.embed`` of this project returns (the reference's ``neck`` output, permuted).  The loss is sum(out * cot), run in
float64 and in float32.

Stored per parameter: ``grad/<name>`` the float64 gradient and ``ref_f32_grad_err/<name>`` = max |float32 run - float64 run|; the
``forward`` run in sam_encoder_grad.npz, the ``embed`` run under the same keys in sam_encoder_grad_embed.npz.  Both runs in float64
are 2.1 MB and no file here may exceed 1 000 000 bytes, so a tensor of 1024 elements or more is stored as a float32 head plus a
float32 remainder (float64 value - head; the sum of the two carries 48 bits of it, far inside the 1e-10 below), and the
remainders go to files of their own: sam_encoder_grad_rem.npz and sam_encoder_grad_embed_rem.npz.  Head and remainder are each
four byte planes (``grad_planes/<name>``, ``grad_rem_planes/<name>``: uint8 [4, n], with ``grad_shape/<name>``; the exponent
bytes side by side compress, the interleaved ones do not); smaller tensors are float64.  tests/vit_grad_ref.py's
``open_fixture`` reads a run's two files as one and ``fixture_grad`` puts the halves together.  The cotangents are multiples of
1/8 in [-2, 2].

Asserted here: tests/vit_grad_ref.py (the backward formulas written out, no autograd) reproduces every float64 gradient to 1e-10,
and each of its four misreadings moves a named gradient by more than 100 x that gradient's bar
max(4 x ref_f32_grad_err, 2^-21 max |gradient|).

    python tests/golden/make_golden_sam_encoder_grad.py /path/to/reference
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

SEED = 20261020
MISREADINGS = (
    ('pad_bias', dict(pad_bias=False), 'blocks.0.attn.qkv.bias'),
    ('rel_in_dq', dict(rel_in_dq=False), 'blocks.1.attn.qkv.weight'),
    ('rel_scaled_q', dict(rel_scaled_q=True), 'blocks.1.attn.rel_pos_h'),
    ('pad_queries', dict(pad_queries=True), 'blocks.0.attn.qkv.weight'),
)


def bar(err, grad):
    return max(4.0 * float(err), 2.0 ** -21 * float(np.abs(grad).max()))


def reference_grads(model, img, cot, embed):
    model.zero_grad()
    kept = []
    hook = model.neck.register_forward_hook(lambda m, i, o: kept.append(o))
    out = model(img)
    hook.remove()
    if embed:
        out = kept[0].permute(0, 2, 3, 1)
    (out * cot.to(out.dtype)).sum().backward()
    return {k: p.grad.detach().clone() for k, p in model.named_parameters()}


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
        final_dim=cfg['final_dim'], downsample_factor=cfg['downsample_factor']).eval()
    model.load_state_dict(wts)
    gen = torch.Generator().manual_seed(SEED)
    # multiples of 1/8 in [-2, 2]: exact in float32, and the file's compression takes them to a byte each
    draw = lambda *shape: torch.randint(-16, 17, shape, generator=gen).float() / 8.0
    cots = {False: draw(2, cfg['out_chans'], 13, 24), True: draw(2, 12, 12, cfg['out_chans'])}

    report = {}
    for embed in (False, True):
        suffix = '_embed' if embed else ''
        data, rem = {'cot': cots[embed].numpy()}, {}
        model.float()
        g32 = reference_grads(model, img.float(), cots[embed], embed)
        model.double()
        g64 = reference_grads(model, img.double(), cots[embed], embed)
        mine = VG.encoder_backward(wts, cfg, img.double(), cots[embed].double(), embed=embed)
        assert set(mine) == set(g64), set(mine) ^ set(g64)
        worst = max(float((mine[k] - g64[k]).abs().max()) for k in g64)
        assert worst <= 1e-10, worst
        errs = {k: float((g32[k].double() - g64[k]).abs().max()) for k in g64}
        for k, g in g64.items():
            if g.numel() < 1024:
                data[f'grad/{k}'] = g.numpy()
            else:
                head = g.float()
                data[f'grad_planes/{k}'] = VG.to_byte_planes(head.numpy())
                rem[f'grad_rem_planes/{k}'] = VG.to_byte_planes((g - head.double()).float().numpy())
                data[f'grad_shape/{k}'] = np.array(g.shape, dtype=np.int64)
            data[f'ref_f32_grad_err/{k}'] = np.float64(errs[k])
        for label, kw, name in MISREADINGS:
            wrong = VG.encoder_backward(wts, cfg, img.double(), cots[embed].double(), embed=embed, **kw)
            moved = float((wrong[name] - g64[name]).abs().max())
            b = bar(errs[name], g64[name].numpy())
            assert moved > 100.0 * b, (label, name, moved, b)
            report[label + suffix] = round(moved / b)
        report['restatement' + suffix] = worst
        for tail, content in (('', data), ('_rem', rem)):
            path = os.path.join(HERE, f'sam_encoder_grad{suffix}{tail}.npz')
            np.savez_compressed(path, **content)
            print(f"wrote {path}: {os.path.getsize(path)} bytes")
            assert os.path.getsize(path) < 1000000
        stored = VG.open_fixture(HERE, embed)
        back = max(float((VG.fixture_grad(stored, k) - g).abs().max()) for k, g in g64.items())
        assert back <= 1e-12, back
    print(report)


if __name__ == '__main__':
    main(sys.argv[1])
