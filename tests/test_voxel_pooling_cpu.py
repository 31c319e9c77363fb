"""CPU: which planned gather kernel the library picks for a problem size (host arithmetic only; nothing touches a device)."""
import pytest

from sgv3d_amd import _lib

VOX, OTHER = 2, 0            # sgv3d_voxel_pooling_kernel_for: the voxel-owner kernel | vp_gather3_kernel or vp_gather_kernel
CFG2 = (1, 1_555_200, 80, 128, 128)                      # B, N, C, X, Y of a cfg-2-like frame


@pytest.fixture
def lib():
    lib = _lib.load()
    yield lib
    assert lib.sgv3d_voxel_pooling_select_kernel(0) == 0


@pytest.mark.parametrize("fused", [0, 1])
def test_kernel_for_follows_channel_count_and_tensor_size(lib, fused):
    assert lib.sgv3d_voxel_pooling_kernel_for(*CFG2, fused) == VOX
    B, N, _, X, Y = CFG2
    for C in (20, 87):                                   # below 24 | not a multiple of 4: vp_gather_kernel
        assert lib.sgv3d_voxel_pooling_kernel_for(B, N, C, X, Y, fused) == OTHER
    # 1 x 14e6 x 80 f32 = 4.48e9 bytes >= 0xfff00000: past the voxel-owner kernel's 32-bit byte offsets
    assert 14_000_000 * 80 * 4 >= 0xFFF00000
    assert lib.sgv3d_voxel_pooling_kernel_for(1, 14_000_000, 80, X, Y, fused) == OTHER
    # ... and so is an output map of 4000 x 4000 x 80 f32 = 5.12e9 bytes, however few the points
    assert lib.sgv3d_voxel_pooling_kernel_for(1, 1000, 80, 4000, 4000, fused) == OTHER


def test_select_kernel_one_forces_the_large_tensor_kernel(lib):
    assert lib.sgv3d_voxel_pooling_select_kernel(1) == 0
    assert lib.sgv3d_voxel_pooling_kernel_for(*CFG2, 0) == OTHER
    assert lib.sgv3d_voxel_pooling_kernel_for(*CFG2, 1) == OTHER
    assert lib.sgv3d_voxel_pooling_select_kernel(2) == 0
    assert lib.sgv3d_voxel_pooling_kernel_for(*CFG2, 0) == VOX
    assert lib.sgv3d_voxel_pooling_select_kernel(1) == 0
    assert lib.sgv3d_voxel_pooling_select_kernel(0) == 0
    assert lib.sgv3d_voxel_pooling_kernel_for(*CFG2, 0) == VOX
    assert lib.sgv3d_voxel_pooling_select_kernel(3) != 0            # rejected, selection unchanged
    assert lib.sgv3d_voxel_pooling_kernel_for(*CFG2, 0) == VOX
