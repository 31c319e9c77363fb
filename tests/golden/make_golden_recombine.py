"""Writes tests/golden/recombine.npz: what the reference's scripts/data_preprocess/recombine_utils.py makes of two synthetic
scenes (40 x 64 and 37 x 61 frames, a destination and three sources each; tests/recombine_util.py builds them).

The module is imported with empty ``sys.modules`` stubs for the libraries it never calls on this path (mmcv, pyquaternion,
tqdm, scripts.data_converter.visual_utils) and a ``cv2`` stub.  Recorded, per scene ``<n>``:

  ``<n>_M`` [3, 3, 3]                ``Robutness.get_M`` per source
  ``<n>_warped`` f32 [1, H, W, 3]    ``transform_with_M_bilinear`` (through ``unify_extrinsic_params_tools``) of the first source,
                                     RGB order; the other sources' warps are pinned through the combined frame
  ``<n>_delta`` [3, 3]               the shift ``unify_extrinsic_params_tools`` added to the corners
  ``<n>_dest_boxes`` / ``<n>_src<s>_boxes`` [n, 4]   ``update_bbox_info``: the float box of every object (NaN where
                                     dropped), in the order the fixture stores the objects
  ``<n>_src<s>_*``                   the source's objects IN THE ORDER OF THE REFERENCE'S DRAW (``random.sample`` inside
                                     ``objects_combine_tools``, seeded): selected objects first as drawn, the others after
  ``<n>_kept<s>`` bool [n]           which of them ``objects_combine_tools`` accepted
  ``<n>_image`` u8 [H, W, 3], ``<n>_mask`` u8 [H, W], ``<n>_beta`` [3]   the combined frame, RGB order
  ``<n>_labels``                     the text ``label_generation`` wrote
  ``iou_a`` [5, 4], ``iou_b`` [4, 4], ``iou_out`` [5, 4]   ``iou`` on hand-made boxes

PATCHED (``patched`` in the fixture says so): ``get_sam_mask`` is the stated stand-in for SAM -- the frame's stored class-id
mask (the source's sampled at the reference's own warp coordinates, nearest neighbour, dead pixels 0), kept inside the
union of the prompt boxes; the destination's is its stored mask.  ``cv2.cvtColor`` and ``cv2.convertScaleAbs`` are served by
the project's restatement (tests/recombine_ref.py); the float gray comes back as float64 holding the float32 values, so
the reference's ``np.mean`` sums it in float64.  Annotations carry a ``score`` key (the reference's loader never sets one,
``label_generation`` reads it when present).

The maker asserts that no warp coordinate lies within 1e-9 of a dead-flag boundary, of an integer or of a half-integer:
the reference's BLAS product cannot flip a pixel against the elementwise restatement.

    python tests/golden/make_golden_recombine.py /path/to/reference
"""
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import recombine_ref as R            # noqa: E402
import recombine_util as U           # noqa: E402

SEED = 20261018
SCENES = {'a': (40, 64, 11), 'b': (37, 61, 12)}


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def _cvt(img, code):
    rgb = img[..., ::-1]
    if img.dtype == np.uint8:
        return R.gray_u8(rgb)
    return R.gray_f32(rgb).astype(np.float64)


def import_reference(root):
    for name in ('mmcv', 'pyquaternion', 'tqdm', 'scripts.data_converter', 'scripts.data_converter.visual_utils'):
        _stub(name)
    sys.modules['pyquaternion'].Quaternion = object
    sys.modules['tqdm'].tqdm = lambda it, *a, **k: it
    _stub('cv2', COLOR_BGR2GRAY=6, cvtColor=_cvt, convertScaleAbs=lambda img, alpha, beta: R.shift_abs(img, beta)[0])
    sys.path.insert(0, root)
    import scripts.data_preprocess.recombine_utils as ref
    return ref


def sample_info(fr):
    o = fr['objects']
    annos = []
    for i, name in enumerate(o['names']):
        c = np.array(o['corners'][i], np.float64)
        annos.append(dict(dim=np.array(o['dim'][i]).astype(float), loc=np.mean(c, axis=-1), rotation=0.0, name=name, box2d=[0, 0, 0, 0],
                          corners_3d=c, truncated_state=float(o['truncated'][i]), occluded_state=float(o['occluded'][i]),
                          score=float(o['score'][i]), uid=i))
    return dict(img=np.ascontiguousarray(fr['image'][..., ::-1]), Tr_ego2cam=np.array(fr['Tr_ego2cam']), P2=np.array(fr['P2']),
                annos_ego=annos, mask_image=None, frame_id="0", split="training", img_path="", height=0.0)


def reference_positions(M, H, W):
    """The warp coordinates as the reference computes them (one BLAS product over all pixels)."""
    xu, yv = np.meshgrid(range(W), range(H))
    uvd = np.stack([xu, yv, np.ones_like(xu)], -1).reshape(-1, 3) * 10.0
    p = np.matmul(np.linalg.inv(M), uvd.T).T
    return (p[:, :2] / p[:, 2:]).reshape(H, W, 2)


def assert_clear(q, H, W):
    for v, hi in ((q[..., 0], W - 2), (q[..., 1], H - 2)):
        inside = (v > -1) & (v < hi + 1)
        gap = np.minimum(np.abs(v * 2 - np.rint(v * 2)) / 2, np.minimum(np.abs(v), np.abs(v - hi)))
        assert gap[inside].min() > 1e-9, "a warp coordinate sits on a boundary: change the scene's seed"


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('SGV3D_REFERENCE', '')
    ref = import_reference(root)
    out = {'patched': np.array("get_sam_mask: stored class-id mask stand-in; cv2.cvtColor, cv2.convertScaleAbs: tests/recombine_ref.py")}
    rob = ref.Robutness()
    for name, (H, W, seed) in SCENES.items():
        dest, sources = U.make_scene(seed, H, W)
        info_d = sample_info(dest)
        infos, Ms, deltas, queue = [], [], [], [np.minimum(dest['mask'], 6)[..., None].astype(np.uint8)]
        for s, src in enumerate(sources):
            info = sample_info(src)
            M = rob.get_M(info["Tr_ego2cam"][:3, :3], info["P2"][:3, :3], info_d["Tr_ego2cam"][:3, :3], info_d["P2"][:3, :3])
            q = reference_positions(M, H, W)
            assert_clear(q, H, W)
            dead = (q[..., 0] < 0) | (q[..., 0] > W - 2) | (q[..., 1] < 0) | (q[..., 1] > H - 2)
            qc = np.stack([np.clip(q[..., 0], 0, W - 2), np.clip(q[..., 1], 0, H - 2)], -1)
            ids = np.minimum(src['mask'][np.floor(qc[..., 1] + 0.5).astype(int), np.floor(qc[..., 0] + 0.5).astype(int)], 6)
            queue.append(np.where(dead, 0, ids)[..., None].astype(np.uint8))
            before = [a['corners_3d'].copy() for a in info['annos_ego']]
            uni = ref.unify_extrinsic_params_tools(rob, info, info_d)
            deltas.append(uni['annos_ego'][0]['corners_3d'][:, 0] - before[0][:, 0] if before else np.zeros(3))
            out.setdefault(f'{name}_warped', []).append(uni['img'][..., ::-1])
            n = len(uni['annos_ego'])
            uni = ref.update_bbox_info(uni)
            boxes = np.full((n, 4), np.nan)
            for a in uni['annos_ego']:
                boxes[a['uid']] = a['bbox']
            out[f'{name}_src{s}_boxes_stored'] = boxes
            infos.append(uni)
            Ms.append(M)

        calls = []

        def standin(predictor, bbox_prompts, bbox_labels, img):
            ids = queue[len(calls)]
            calls.append(1)
            if len(calls) == 1:
                return ids                                      # the destination: its stored mask
            keep = np.zeros((H, W, 1), bool)
            for x0, y0, x1, y1 in np.asarray(bbox_prompts).reshape(-1, 4).tolist():
                keep[int(y0):int(y1) + 1, int(x0):int(x1) + 1] = True
            return np.clip(np.where(keep, ids, 0), 0, 6).astype(np.uint8)

        draws = []
        orig = random.sample

        def recording_sample(population, k):
            got = orig(population, k)
            draws.append([a['uid'] for a in got])
            return got

        ref.get_sam_mask = standin
        random.sample = recording_sample
        random.seed(SEED)
        n_dest = len(info_d['annos_ego'])
        try:
            comb = ref.objects_combine_tools(None, infos, info_d, 1.0)
        finally:
            random.sample = orig
        assert len(calls) == 4 and len(draws) == 3
        dboxes = np.full((n_dest, 4), np.nan)
        for a in dest_annos(comb, infos):
            dboxes[a['uid']] = [float(v) for v in a['bbox']]
        out[f'{name}_dest_boxes'] = dboxes
        U.save_frame(out, f'{name}_dest', dest)
        for s, src in enumerate(sources):
            n = len(src['objects']['names'])
            order = draws[s] + [i for i in range(n) if i not in draws[s]]
            U.save_frame(out, f'{name}_src{s}', src, order)
            out[f'{name}_src{s}_boxes'] = out.pop(f'{name}_src{s}_boxes_stored')[order]
            accepted = {a['uid'] for a in comb['annos_ego'] if any(a is b for b in infos[s]['annos_ego'])}
            out[f'{name}_kept{s}'] = np.array([i in accepted for i in order])
        out[f'{name}_n_src'] = np.array(len(sources))
        out[f'{name}_M'], out[f'{name}_delta'] = np.array(Ms), np.array(deltas)
        out[f'{name}_warped'] = np.array(out[f'{name}_warped'][:1], np.float32)      # the first source's: the others show in the frame
        out[f'{name}_image'] = np.ascontiguousarray(comb['img'][..., ::-1]).astype(np.uint8)
        out[f'{name}_mask'] = comb['mask_image'][..., 0].astype(np.uint8)
        bd = np.mean(_cvt(info_d['img'], 6))
        out[f'{name}_beta'] = np.array([R.beta_of(bd, np.mean(_cvt(i['img'], 6))) for i in infos])
        path = os.path.join(HERE, '_recombine_labels.txt')
        ref.label_generation(comb['Tr_ego2cam'], comb['annos_ego'], path)
        out[f'{name}_labels'] = np.array(open(path).read())
        os.remove(path)

    a = np.array([[0, 0, 10, 10], [2.5, 3, 8, 20.25], [0, 0, 0, 0], [5, 5, 6, 6], [-3, -2, 4.5, 30]], np.float64)
    b = np.array([[1, 1, 9, 9], [0, 0, 10, 10], [20, 20, 30, 30], [3, 2, 7, 19]], np.float64)
    out['iou_a'], out['iou_b'], out['iou_out'] = a, b, ref.iou(a, b)
    np.savez_compressed(os.path.join(HERE, 'recombine.npz'), **out)


def dest_annos(comb, infos):
    """The destination's own annotations that survived ``update_bbox_info``: the combined list minus the sources'."""
    from_sources = [a for i in infos for a in i['annos_ego']]
    return [a for a in comb['annos_ego'] if not any(a is b for b in from_sources)]


if __name__ == '__main__':
    main()
