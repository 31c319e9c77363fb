"""GPU: the training-time augmentation launches (csrc/augment.hip) bit-exact against the reference's Pillow outputs
(tests/golden/train_augment.npz) and against the numpy restatement (tests/train_augment_ref.py) at full size, the
no-augmentation frames against ImagePreprocessor, a training step fed through them, and argument errors."""
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import preprocess_ref as P
import train_augment_ref as R
from sgv3d_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IMG_CONF = dict(img_mean=[123.675, 116.28, 103.53], img_std=[58.395, 57.12, 57.375], to_rgb=True)
UNIT_CONF = dict(img_mean=[0.0, 0.0, 0.0], img_std=[1.0, 1.0, 1.0], to_rgb=False)   # float output = the uint8 values


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "train_augment.npz"))


def _aug(src_hw, final_dim, img_conf=IMG_CONF):
    from sgv3d_amd.train_augment import TrainAugmenter
    return TrainAugmenter({'final_dim': final_dim, 'bot_pct_lim': (0.0, 0.0)}, img_conf, src_hw=src_hw, device=DEV)


def _placed(ie, ratio, roll, tp, center, bright=None, u=None):
    from sgv3d_amd.train_augment import AugmentParams
    n = len(ie)
    return AugmentParams(ie, ratio, roll, [0.0] * n, bright or [False] * n, u or [0.0] * n, center=center,
                         transform_pitch=tp)


def _fixture_params(d, names):
    args = [d[f'{n}_args'] for n in names]
    centers = [tuple(int(v) for v in d[f'{n}_intrin'][:2, 2].astype(np.int32)) for n in names]
    return _placed([True] * len(names), [a[0] for a in args], [a[1] for a in args], [int(a[2]) for a in args], centers)


@pytest.mark.parametrize("hw", [(90, 160), (135, 240), (108, 192)])
def test_images_bit_exact_against_pillow(fixture, hw):
    """Every fixture case of one source size in one batch; the eval resize is the identity (final size = source size) and
    the normalise a unit one, so the output is the rectified frame itself."""
    names = [n for n in ('down', 'up', 'one_axis', 'large_kernel', 'unit', 'pitch_off')
             if fixture[f'{n}_src'].shape[:2] == hw]
    src = np.stack([fixture[f'{n}_src'] for n in names])
    imgs, _ = _aug(hw, hw, UNIT_CONF)(torch.from_numpy(src).to(DEV), _fixture_params(fixture, names))
    got = imgs.cpu().numpy()
    for i, n in enumerate(names):
        want = fixture[f'{n}_out'].transpose(2, 0, 1).astype(np.float32)
        assert np.array_equal(got[i, 0, 0], want), f"{n}: {(got[i, 0, 0] != want).sum()} values differ"


def test_mask_bit_exact_against_pillow(fixture):
    src = fixture['mask_src']
    aug = _aug(src.shape[:2], src.shape[:2])
    masks = torch.from_numpy(np.stack([src, src])).to(DEV)
    p = _fixture_params(fixture, ['mask', 'mask'])
    p.ie[1] = False                                          # and one mask that is only resized
    got = aug.mask(masks, p).cpu().numpy()
    assert np.array_equal(got[0, 0], P.mask_labels(fixture['mask_out']))
    assert np.array_equal(got[1, 0], P.mask_labels(src))


def _full_params():
    """Four sampled frames at 1080 x 1920 covering rectified + jittered, rectified only, jittered only, neither."""
    from sgv3d_amd.train_augment import augment_camera, sample_params
    p = sample_params(4, random.Random(11), np.random.RandomState(11))
    p.ie[:] = [True, True, False, False]
    p.bright[:] = [True, False, True, False]
    p.u[:] = [0.83, 0.0, 0.41, 0.0]
    p.ratio[:2], p.roll_deg[:2], p.pitch_deg[:2] = [0.87, 1.27], [1.7, -2.2], [0.4, -0.9]
    mats = S.make_mats(4)
    for i in range(4):
        augment_camera(dict(sensor2ego=mats['sensor2ego_mats'][i, 0, 0].numpy(),
                            intrin=mats['intrin_mats'][i, 0, 0].numpy()), p, i)
    return p


def _restated(frame, p, i, aug, img_conf=IMG_CONF):
    img = frame
    if p.ie[i]:
        K = np.eye(4)
        K[:2, 2] = p.center[i]
        img = R.intrin_extrin_transform(img, p.ratio[i], p.roll_deg[i], int(p.transform_pitch[i]), K)
    img = P.transform(img, aug.pre.resize_dims, aug.pre.crop, False)
    if p.bright[i]:
        img = R.brightness(img, p.u[i])
    return P.normalize(img, img_conf['img_mean'], img_conf['img_std'], img_conf['to_rgb'])


def test_full_size_matches_restatement():
    """1080x1920 -> 864x1536 (the shipped DAIR configs), batch 4 in [B, S, N, H, W, 3] form."""
    p = _full_params()
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:1080, 0:1920]
    base = (128 + 90 * np.sin(xx / 37.0 + yy / 23.0))[None, ..., None]
    src = np.clip(base + rng.integers(-60, 61, (4, 1080, 1920, 3)), 0, 255).astype(np.uint8)
    aug = _aug((1080, 1920), (864, 1536))
    imgs, ida = aug(torch.from_numpy(src).to(DEV).view(2, 1, 2, 1080, 1920, 3), p)
    assert imgs.shape == (2, 1, 2, 3, 864, 1536) and ida.shape == (2, 1, 2, 4, 4)
    got = imgs.view(4, 3, 864, 1536).cpu().numpy()
    for i in range(4):
        want = _restated(src[i], p, i, aug)
        assert np.array_equal(got[i], want), f"frame {i}: {(got[i] != want).sum()} values differ"


def test_unaugmented_frames_are_the_preprocessor():
    from sgv3d_amd.preprocess import ImagePreprocessor
    hw, fd = (90, 160), (72, 128)
    frames = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (3,) + hw + (3,), dtype=np.uint8)).to(DEV)
    p = _placed([False] * 3, [1.0] * 3, [0.0] * 3, [0] * 3, [(80, 45)] * 3)
    got, ida = _aug(hw, fd)(frames, p)
    want, wida = ImagePreprocessor({'final_dim': fd}, IMG_CONF, src_hw=hw, device=DEV)(frames)
    assert torch.equal(got, want) and torch.equal(ida, wida)


def test_training_step_on_augmented_frames():
    """A small-config training step fed TrainAugmenter's images and augment_camera's matrices: finite loss, and the same
    loss bits as the step fed the restatement's tensors."""
    from sgv3d_amd.input_contract import collate_mats
    from sgv3d_amd.models.bev_height import BEVHeight
    from sgv3d_amd.train_augment import augment_camera, sample_params
    B, hw = 2, (160, 240)                                    # -> 128 x 192 at the DAIR ratio 0.8
    bconf, hconf = S.small_conf()
    aug = _aug(hw, bconf['final_dim'])
    p = sample_params(B, random.Random(3), np.random.RandomState(3))
    p.ie[:], p.bright[:], p.u[:] = True, [True, False], [0.6, 0.0]
    p.ratio[:], p.roll_deg[:], p.pitch_deg[:] = [0.92, 1.12], [1.1, -0.8], [0.3, -0.5]
    base = S.make_mats(B, scale=hw[0] / 1080)
    cams = []
    for i in range(B):
        cams.append(augment_camera(dict(sensor2ego=base['sensor2ego_mats'][i, 0, 0].numpy(),
                                        intrin=base['intrin_mats'][i, 0, 0].numpy(), ida=aug.ida, bda=np.eye(4)), p, i))
    mats = collate_mats(cams, DEV)
    frames = np.random.default_rng(9).integers(0, 256, (B,) + hw + (3,), dtype=np.uint8)
    imgs, ida = aug(torch.from_numpy(frames).to(DEV), p)
    want = torch.from_numpy(np.stack([_restated(frames[i], p, i, aug) for i in range(B)])).view(imgs.shape)
    assert torch.equal(imgs.cpu(), want)
    assert torch.equal(ida, mats['ida_mats'])
    boxes, labels = S.make_gt(B, seed=1, n_range=(6, 12), stress=False)
    for b in boxes:
        b[:, 0] *= 0.25
        b[:, 1] *= 0.25

    def step(x):
        torch.manual_seed(0)
        model = BEVHeight(bconf, hconf)
        S.randomize_norm_stats_(model, seed=0)
        for m in model.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
        model = model.to(DEV).train()
        model.head.train_cfg = dict(model.head.train_cfg, grid_size=[256, 256, 1],
                                    point_cloud_range=[0, -12.8, -5, 25.6, 12.8, 3])
        targets = model.get_targets([b.to(DEV) for b in boxes], [l.to(DEV) for l in labels])
        loss = model.loss(targets, model(x, mats))
        loss.backward()
        return loss.detach().cpu()

    a, b = step(imgs), step(want.to(DEV))
    # identical inputs: the two steps differ only by the order of the training kernels' float atomics, if at all
    assert torch.isfinite(a) and abs(float(a) - float(b)) <= 1e-6 * abs(float(b)), (float(a), float(b))


def test_rejects_bad_input():
    aug = _aug((90, 160), (72, 128))
    frames = torch.zeros(2, 90, 160, 3, dtype=torch.uint8, device=DEV)
    ok = _placed([True, False], [0.9, 1.0], [1.0, 0.0], [0, 0], [(80, 45)] * 2)
    with pytest.raises(ValueError, match="> 0"):
        aug(frames, _placed([True, True], [0.9, 0.005], [1.0, 0.0], [0, 0], [(80, 45)] * 2))
    with pytest.raises(ValueError, match="parameter sets"):
        aug(frames[:1], ok)
    with pytest.raises(ValueError, match="CUDA"):
        aug(frames.cpu(), ok)
    with pytest.raises(ValueError, match="uint8"):
        aug(frames.float(), ok)
    with pytest.raises(ValueError, match="90x160"):
        aug(torch.zeros(2, 91, 160, 3, dtype=torch.uint8, device=DEV), ok)
    imgs, _ = aug(frames, ok)                                # a valid call still works after the rejected ones
    torch.cuda.synchronize()
    assert imgs.shape == (2, 1, 1, 3, 72, 128)
