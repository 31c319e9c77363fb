"""Writes tests/golden/sam_encoder.npz: what the reference's layers/backbones/sam_encoder.py computes for one small model.

The reference module is imported with a ``cv2`` stub (it imports cv2 and never calls it) and with ``layers`` /
``layers.backbones`` as bare packages, so that ``layers/__init__.py`` (which pulls mmdet3d) never runs.  The model is
tests/vit_ref.py's FIXTURE_CFG: 96 x 96 input, 8 x 8 patches -> 12 x 12 tokens, 64 channels, 2 heads of 32, a windowed
block (window 5: the map pads to 15 x 15, every edge window holds bias tokens) and a global block, rel-pos on, eps 1e-6,
final_dim (864, 1536) / 64 -> the crop to 9 x 12 (the map is narrower than the crop's 16) and the resize to 13 x 24 both
work.  The input is [2, 3, 54, 96] with uint8 values: 54 is no multiple of 8, a patch row straddles the image edge.

Weights: torch's default initialisation (seeded), then pos_embed and the rel-pos tables N(0, 0.2), every bias N(0, 0.5),
every norm weight U(0.5, 1.5) -- all float32, so that the float64 run sees float32-representable parameters.

Stored: ``w/<name>`` the state dict (f32), ``input`` (u8), ``out`` the float64 output, ``block<i>`` the float64 output of
each block, ``ref_f32_err`` max |float32 run - float64 run| of the reference itself, ``vit_b_names`` / ``vit_b_shapes`` the
parameter list of ``build_sam_vit_b((864, 1536), 16)``.

Asserted here: tests/vit_ref.py reproduces the reference to 1e-12, and each of the three misreadings it can switch on
(padding keys masked, padding tokens zero, scaled q in the rel-pos terms) moves the output by more than 1e-2.

    python tests/golden/make_golden_sam_encoder.py /path/to/reference
"""
import importlib
import json
import os
import sys
import types
from functools import partial

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import vit_ref as V          # noqa: E402

SEED = 20261019


def import_reference(root):
    sys.modules['cv2'] = types.ModuleType('cv2')
    for name in ('layers', 'layers.backbones'):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(root, *name.split('.'))]
        sys.modules[name] = pkg
    return importlib.import_module('layers.backbones.sam_encoder')


def main(root):
    ref = import_reference(root)
    cfg = V.FIXTURE_CFG
    torch.manual_seed(SEED)
    model = ref.ImageEncoderViT(
        img_size=cfg['img_size'], patch_size=cfg['patch_size'], embed_dim=cfg['embed_dim'], depth=cfg['depth'],
        num_heads=cfg['num_heads'], out_chans=cfg['out_chans'], window_size=cfg['window_size'],
        global_attn_indexes=cfg['global_attn_indexes'], use_rel_pos=True, norm_layer=partial(torch.nn.LayerNorm, eps=cfg['eps']),
        final_dim=cfg['final_dim'], downsample_factor=cfg['downsample_factor']).eval()
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name == 'pos_embed' or 'rel_pos' in name:
                p.normal_(0.0, 0.2)
            elif name.endswith('bias'):
                p.normal_(0.0, 0.5)
            elif 'norm' in name or name in ('neck.1.weight', 'neck.3.weight'):
                p.uniform_(0.5, 1.5)
    img = torch.randint(0, 256, (2, 3, 54, 96), generator=torch.Generator().manual_seed(SEED + 1)).to(torch.uint8)
    wts = {k: v.clone() for k, v in model.state_dict().items()}

    with torch.no_grad():
        out32 = model(img.float())
        model.double()
        blocks = []
        hooks = [b.register_forward_hook(lambda m, i, o: blocks.append(o.clone())) for b in model.blocks]
        out64 = model(img.double())
        for h in hooks:
            h.remove()
        ref_err = float((out32.double() - out64).abs().max())

        mine_blocks = []
        mine = V.encoder_forward(wts, cfg, img.double(), mine_blocks)
    assert tuple(out64.shape) == (2, cfg['out_chans'], 13, 24), out64.shape
    assert float((mine - out64).abs().max()) <= 1e-12, float((mine - out64).abs().max())
    for a, b in zip(mine_blocks, blocks):
        assert float((a - b).abs().max()) <= 1e-12
    moved = {}
    with torch.no_grad():
        for label, kw in (('masked', dict(pad_keys='masked')), ('zero', dict(pad_keys='zero')), ('scaled_q', dict(rel_uses_scaled_q=True))):
            moved[label] = float((V.encoder_forward(wts, cfg, img.double(), **kw) - out64).abs().max())
            assert moved[label] > 1e-2, (label, moved[label])

    vit_b = ref.build_sam_vit_b((864, 1536), 16)
    names = [k for k, _ in vit_b.named_parameters()]
    shapes = [list(v.shape) for _, v in vit_b.named_parameters()]

    data = {'w/' + k: v.numpy() for k, v in wts.items()}
    data.update(input=img.numpy(), out=out64.numpy(), ref_f32_err=np.float64(ref_err),
                vit_b_names=np.array(json.dumps(names)), vit_b_shapes=np.array(json.dumps(shapes)))
    for i, b in enumerate(blocks):
        data[f'block{i}'] = b.numpy()
    path = os.path.join(HERE, 'sam_encoder.npz')
    np.savez_compressed(path, **data)
    print(f"wrote {path}: {os.path.getsize(path)} bytes; max |out| {float(out64.abs().max()):.3f}; reference f32 error {ref_err:.3e}; "
          f"misreadings move the output by {moved}")
    assert os.path.getsize(path) < 1000000


if __name__ == '__main__':
    main(sys.argv[1])
