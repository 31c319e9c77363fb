"""The annotate path end to end on synthetic frames (no dataset is needed): camera files -> ``JpegDecoder`` -> ``ImagePreprocessor``
-> the small model with heads that fire -> ``decode_device`` -> ``DetectionRenderer.draw_packed`` -> ``JpegEncoder`` -> files.
Only the encoded files cross PCIe, in and out.

    python tools/render_demo.py --out /tmp/render_demo [--frames 2]
writes NNNNNN_cam.jpg and NNNNNN_bev.jpg per frame and prints one JSON line with what was drawn."""
import argparse
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sgv3d_amd import hip_ops, render, synthetic as S  # noqa: E402
from sgv3d_amd.jpeg import JpegDecoder  # noqa: E402
from sgv3d_amd.jpeg_encode import JpegEncoder  # noqa: E402
from sgv3d_amd.preprocess import ImagePreprocessor  # noqa: E402

SRC_HW, FINAL = (270, 480), (128, 192)
IMG_CONF = dict(img_mean=[123.675, 116.28, 103.53], img_std=[58.395, 57.12, 57.375], to_rgb=True)


def camera_files(n):
    """Synthetic camera frames, encoded on the host as a camera would deliver them."""
    from PIL import Image
    rng = np.random.default_rng(11)
    y, x = np.mgrid[0:SRC_HW[0], 0:SRC_HW[1]]
    files = []
    for i in range(n):
        img = np.stack([100 + 50 * np.sin(x / (41.0 + i)), 120 + 0.2 * y, 150 - 0.1 * x], -1) + rng.normal(0, 5, SRC_HW + (3,))
        buf = io.BytesIO()
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(buf, format='JPEG', quality=90)
        files.append(buf.getvalue())
    return files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--frames', type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "render_demo needs the GPU (there is no CPU path)"
    from sgv3d_amd.models.bev_height import BEVHeight
    dev, n = torch.device('cuda:0'), args.frames
    bc, hc = S.small_conf(final=FINAL, bev=64, depth=18)
    hc['bbox_coder'] = dict(hc['bbox_coder'], pc_range=[0, -12.8, -5, 25.6, 12.8, 3], post_center_range=[0.0, -15.0, -10.0, 30.0, 15.0, 10.0],
                            max_num=100)
    hc['test_cfg'] = dict(hc['test_cfg'], post_center_limit_range=[0.0, -15.0, -10.0, 30.0, 15.0, 10.0], post_max_size=20)
    hip_ops.AUTOTUNE = False
    torch.manual_seed(0)
    m = BEVHeight(bc, hc).eval()
    S.checkpoint_like_(m, 2)
    with torch.no_grad():
        for t in m.head.task_heads:                                  # untrained heads: make them fire
            t.heatmap[1].weight.mul_(40.0)
            t.heatmap[1].bias.fill_(-1.0)
            t.dim[1].weight.mul_(3.0)
            t.dim[1].bias.fill_(0.6)
            t.height[1].bias.fill_(-0.5)
    m = m.to(dev)
    m.graph_forward = False
    scale = SRC_HW[1] / 1920.0                                       # the roadside camera's matrix at this frame size
    cams = [S.make_calib(pitch_deg=11.0 + i, cam_h=5.5 + 0.3 * i, fx=2183.375 * scale, fy=2329.2976 * scale, cx=940.59 * scale,
                         cy=567.568 * scale) for i in range(n)]
    t = lambda k: torch.from_numpy(np.stack([c[k] for c in cams])).view(n, 1, 1, 4, 4).to(dev)
    dec = JpegDecoder(src_hw=SRC_HW, device=dev)
    pre = ImagePreprocessor({'final_dim': FINAL, 'bot_pct_lim': (0.0, 0.0)}, IMG_CONF, src_hw=SRC_HW, device=dev)
    frames = dec(camera_files(n))                                    # uint8 [n, H, W, 3] on the GPU
    imgs, ida = pre(frames)
    mats = {'sensor2ego_mats': t('sensor2ego'), 'intrin_mats': t('intrin'), 'ida_mats': ida,
            'sensor2sensor_mats': torch.eye(4, device=dev).view(1, 1, 1, 4, 4).repeat(n, 1, 1, 1, 1), 'sensor2virtual_mats': t('sensor2virtual'),
            'reference_heights': torch.tensor([float(c['reference_height']) for c in cams], device=dev).view(n, 1, 1),
            'bda_mat': torch.eye(4, device=dev).repeat(n, 1, 1)}
    with torch.no_grad():
        packed = m.head.decode_device(m(imgs, mats))
    # the frames are drawn as they were shot: their own camera matrix, not the resized and cropped one the model sees
    calib = [(np.linalg.inv(c['sensor2ego'].astype(np.float64))[:3], c['intrin'][:3, :3].astype(np.float64)) for c in cams]
    canvas = render.BevCanvas(side_range=(-15, 15), fwd_range=(0, 30), res=0.1)
    r = render.DetectionRenderer(S.CLASSES, src_hw=SRC_HW, max_boxes=128, bev=canvas, score_threshold=0.1)
    out = r.draw_packed(frames, packed, [dict(token=f'{i:06d}') for i in range(n)], calib=calib, out=frames)
    cam_files = JpegEncoder(src_hw=SRC_HW, quality=95, max_bytes=1 << 20, device=dev)(out.frames).files()
    bev_files = JpegEncoder(src_hw=(canvas.height, canvas.width), quality=95, max_bytes=1 << 20, device=dev)(out.bev).files()
    os.makedirs(args.out, exist_ok=True)
    for i, (c, b) in enumerate(zip(cam_files, bev_files)):
        for name, data in ((f'{i:06d}_cam.jpg', c), (f'{i:06d}_bev.jpg', b)):
            with open(os.path.join(args.out, name), 'wb') as fp:
                fp.write(data)
    print(json.dumps(dict(frames=n, status=out.status().tolist(), cam_kb=[round(len(f) / 1e3, 1) for f in cam_files],
                          bev_lit_pixels=[int(v) for v in out.bev.any(-1).flatten(1).sum(1).tolist()], out=args.out)))


if __name__ == '__main__':
    main()
