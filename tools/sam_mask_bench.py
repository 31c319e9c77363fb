"""Times the SAM mask stage on the device against tests/sam_ref.py in float32 through torch on the same GPU.

    python tools/sam_mask_bench.py [--out profiles/sam_mask_bench.json] [--model vit_h] [--boxes 20]

One process, HIP events, the median of 10 calls after 3 warm-up calls, the device path and the baseline alternating.  Setup:
``build_sam_vit_h`` with random weights, one 1080 x 1920 frame, 20 boxes.  Reported separately: ``set_image`` (resize, normalise, pad,
encode; the baseline encodes the already resized frame), decoder + compose (boxes to the class-id image; the baseline adds both
``F.interpolate`` calls, the threshold and the paint loop in torch), and the attention launches alone in both regimes.

A kernel trace is a run of its own, without counters:
    rocprofv3 --kernel-trace --stats -d /tmp/sam_trace -- python tools/sam_mask_bench.py --out /tmp/sam_mask_bench_traced.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARMUP, REPEATS = 3, 10
VITS = {"vit_h": (1280, 32, 16, (7, 15, 23, 31)), "vit_l": (1024, 24, 16, (5, 11, 17, 23)), "vit_b": (768, 12, 12, (2, 5, 8, 11))}


def alternate(device_fn, torch_fn):
    """Median, min and max in ms of each of two callables, called in turn."""
    times = ([], [])
    for i in range(WARMUP + REPEATS):
        for j, fn in enumerate((device_fn, torch_fn)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= WARMUP:
                times[j].append(a.elapsed_time(b))
    row = {}
    for name, t in zip(("device", "torch_f32"), times):
        row[name + "_ms"] = statistics.median(t)
        row[name + "_ms_min_max"] = [min(t), max(t)]
    row["speedup"] = row["torch_f32_ms"] / row["device_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam_mask_bench.json"))
    ap.add_argument("--model", default="vit_h", choices=sorted(VITS))
    ap.add_argument("--boxes", type=int, default=20)
    args = ap.parse_args()
    import sam_ref
    from sgv3d_amd import sam_masks
    from sgv3d_amd.segment_anything import SamPredictor, ops, sam_model_registry
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    sam = sam_model_registry[args.model]()
    embed_dim, depth, heads, global_idx = VITS[args.model]
    ref = sam_ref.build(img_size=1024, patch_size=16, embed_dim=embed_dim, depth=depth, num_heads=heads, window_size=14,
                        global_attn_indexes=global_idx)
    sam_ref.randomize_(ref, 0)
    sam.load_state_dict(ref.state_dict(), strict=True)
    sam, ref = sam.to(dev), ref.to(dev).float()
    pred = SamPredictor(sam)
    rng = np.random.default_rng(0)
    h, w, n = 1080, 1920, args.boxes
    yy, xx = np.mgrid[0:h, 0:w]
    frame = np.clip(np.stack([127 + 100 * np.sin(xx / (40.0 + 9 * c)) * np.cos(yy / (55.0 + 7 * c)) for c in range(3)], -1)
                    + rng.normal(0, 20, (h, w, 3)), 0, 255).astype(np.uint8)
    dframe = torch.from_numpy(frame).to(dev)
    x0, y0 = rng.integers(0, w - 400, n), rng.integers(0, h - 300, n)
    boxes = torch.tensor(np.stack([x0, y0, x0 + rng.integers(60, 400, n), y0 + rng.integers(40, 300, n)], 1))
    labels = [int(v) for v in rng.integers(1, 7, n)]
    out = {"gpu": torch.cuda.get_device_name(0), "warmup": WARMUP, "repeats": REPEATS, "model": args.model, "frame": [h, w], "boxes": n,
           "baseline": "tests/sam_ref.py in float32 through torch on the same GPU, alternated with the device path"}

    with torch.no_grad():
        # set_image
        pred.set_image(dframe)
        resized = ops.resize_bilinear_u8(dframe.unsqueeze(0), pred.input_size)
        emb_ref = [None]

        def torch_encode():
            emb_ref[0] = ref.image_encoder(resized)
        out["set_image"] = alternate(lambda: pred.set_image(dframe), torch_encode)
        out["set_image"]["max_abs_diff_to_torch_f32"] = float((pred._features - emb_ref[0]).abs().max())

        # decoder + compose
        tb = pred.transform.apply_boxes_torch(boxes, (h, w)).to(dev)
        lab = torch.tensor(labels, dtype=torch.int32, device=dev)
        fob = torch.zeros(n, dtype=torch.int32, device=dev)
        got, want = [None], [None]

        def device_masks():
            got[0] = pred.class_masks(tb, lab, fob)

        def torch_masks():
            low, _ = ref.low_res(emb_ref[0], tb, [0] * n)
            m = sam_ref.postprocess_masks(low, 1024, pred.input_size, (h, w))[:, 0] > 0
            img = torch.zeros(h, w, device=dev)
            for i in range(n):
                img += m[i] * float(labels[i]) * (img == 0)
            want[0] = img.clamp(0, 6).to(torch.uint8)
        out["decoder_and_compose"] = alternate(device_masks, torch_masks)
        out["decoder_and_compose"]["pixels_differing_from_torch_f32"] = int((got[0][0] != want[0]).sum())
        out["decoder_and_compose"]["class_pixels"] = int((got[0] > 0).sum())
        out["get_sam_mask_end_to_end"] = alternate(lambda: sam_masks.get_sam_mask(pred, boxes, labels, dframe),
                                                   lambda: (torch_encode(), torch_masks()))

        # the attention launches alone: token-to-image (7 queries on 4096 keys) and image-to-token (4096 queries on 7 keys)
        out["attention"] = []
        for nq, nk in ((7, 4096), (4096, 7)):
            q, k, v = torch.randn(n, nq, 128, device=dev), torch.randn(n, nk, 128, device=dev), torch.randn(n, nk, 128, device=dev)
            sp = lambda t: t.reshape(n, -1, 8, 16).transpose(1, 2)

            def torch_attention():
                a = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) / 4.0, -1) @ sp(v)
                return a.transpose(1, 2).reshape(n, nq, 128)
            row = alternate(lambda: ops.sam_attention(q, k, v, 8), torch_attention)
            row["shape"] = {"batch": n, "nq": nq, "nk": nk, "heads": 8, "head_dim": 16}
            row["bytes_moved"] = 4 * 128 * n * (2 * nq + 2 * nk)
            row["device_gb_per_s"] = row["bytes_moved"] / row["device_ms"] / 1e6
            row["max_abs_diff_to_torch_f32"] = float((ops.sam_attention(q, k, v, 8) - torch_attention()).abs().max())
            out["attention"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) else {a: b for a, b in v.items() if a in ("device_ms", "torch_f32_ms", "speedup")})
                      for k, v in out.items() if k != "attention"}))
    for row in out["attention"]:
        print(json.dumps(row))


if __name__ == "__main__":
    main()
