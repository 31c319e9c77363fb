"""Writes tests/golden/sam_encoder_bf16.npz: the yardstick of the encoder's bf16 mode -- what the reference's
layers/backbones/sam_encoder.py computes for the fixture model of sam_encoder.npz under bf16 autocast.

The weights (``w/<name>``) and the input of tests/golden/sam_encoder.npz are loaded into the reference's ``ImageEncoderViT`` (imported
as make_golden_sam_encoder.py does) and the model is run on the CPU under ``torch.autocast('cpu', dtype=torch.bfloat16)``: the mode
the reference's Lightning harness trains and evaluates in (``--amp_backend native``), and the storage this project's bf16 mode keeps
between the layers of a block.

Stored: ``out`` the autocast output (as float32), ``max_abs`` and ``rel_l2`` its maximum absolute and relative-L2 error against the
float64 ``out`` of sam_encoder.npz, ``rms`` the rms of that float64 output.  The model test reads its bar (1.5 x these two errors) from
this file.

Asserted here: each of the three misreadings tests/vit_ref.py can switch on (padding keys masked, padding tokens zero, scaled q in
the rel-pos terms) moves the float64 output by more than 3 x the model test's bar (3 x 1.5 x ``max_abs``).

    python tests/golden/make_golden_sam_encoder_bf16.py /path/to/reference
"""
import os
import sys
from functools import partial

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import vit_ref as V                                          # noqa: E402
from make_golden_sam_encoder import import_reference         # noqa: E402


def main(root):
    ref = import_reference(root)
    cfg = V.FIXTURE_CFG
    base = np.load(os.path.join(HERE, 'sam_encoder.npz'))
    wts = {k[2:]: torch.from_numpy(base[k]) for k in base.files if k.startswith('w/')}
    model = ref.ImageEncoderViT(
        img_size=cfg['img_size'], patch_size=cfg['patch_size'], embed_dim=cfg['embed_dim'], depth=cfg['depth'],
        num_heads=cfg['num_heads'], out_chans=cfg['out_chans'], window_size=cfg['window_size'],
        global_attn_indexes=cfg['global_attn_indexes'], use_rel_pos=True, norm_layer=partial(torch.nn.LayerNorm, eps=cfg['eps']),
        final_dim=cfg['final_dim'], downsample_factor=cfg['downsample_factor']).eval()
    model.load_state_dict(wts)
    img = torch.from_numpy(base['input'])
    out64 = torch.from_numpy(base['out'])
    with torch.no_grad(), torch.autocast('cpu', dtype=torch.bfloat16):
        out = model(img.float())
    out = out.float()
    assert tuple(out.shape) == tuple(out64.shape)
    err = out.double() - out64
    max_abs = float(err.abs().max())
    rel_l2 = float(err.norm() / out64.norm())
    rms = float(out64.pow(2).mean().sqrt())

    bar = 1.5 * max_abs
    moved = {}
    with torch.no_grad():
        for label, kw in (('masked', dict(pad_keys='masked')), ('zero', dict(pad_keys='zero')), ('scaled_q', dict(rel_uses_scaled_q=True))):
            moved[label] = float((V.encoder_forward(wts, cfg, img.double(), **kw) - out64).abs().max())
            assert moved[label] > 3.0 * bar, (label, moved[label], bar)

    path = os.path.join(HERE, 'sam_encoder_bf16.npz')
    np.savez_compressed(path, out=out.numpy(), max_abs=np.float64(max_abs), rel_l2=np.float64(rel_l2), rms=np.float64(rms))
    print(f"wrote {path}: {os.path.getsize(path)} bytes; autocast against float64: max abs {max_abs:.3e}, relative L2 {rel_l2:.3e}, "
          f"output rms {rms:.3f}; misreadings move the output by {moved} (model bar {bar:.3e})")
    assert os.path.getsize(path) < 1000000


if __name__ == '__main__':
    main(sys.argv[1])
