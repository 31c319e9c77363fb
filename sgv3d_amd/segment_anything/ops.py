"""Thin calls of the C ABI of csrc/sam_decoder.hip on torch device tensors.  No CPU path: everything raises before a launch
for a CPU tensor, a tensor that requires grad, or a missing library."""
import ctypes

import numpy as np
import torch

from .. import _lib

COMPOSE_CLASS, COMPOSE_BOOL, COMPOSE_LOGIT = 0, 1, 2
FILTER_BILINEAR = 2


def require_f32(t, what):
    """The house rule (layers/backbones/common.require_device) for a contiguous float32 device tensor."""
    if not isinstance(t, torch.Tensor):
        raise _lib.SGV3DError(f"{what}: a tensor is expected")
    if t.requires_grad and torch.is_grad_enabled():
        raise _lib.SGV3DError(f"{what} is inference only: the input requires grad and there is no backward; "
                              "call it under torch.no_grad() or on a detached tensor")
    if not t.is_cuda:
        raise _lib.SGV3DError(f"{what}: the input must be a tensor on the GPU (there is no CPU fallback)")
    if t.dtype != torch.float32:
        raise _lib.SGV3DError(f"{what}: float32 input expected, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.SGV3DError(f"{what}: a contiguous tensor is expected")


def _rows(t, what):
    """(tensor, batch, rows, row stride) of a [B, N, C] tensor whose last dimension is dense and whose batches are N rows apart."""
    if t.dim() != 3 or t.stride(2) != 1 or t.stride(0) != t.shape[1] * t.stride(1):
        raise _lib.SGV3DError(f"sam_attention: {what} must be [B, N, C] rows with one row stride, got shape {tuple(t.shape)} "
                              f"strides {t.stride()}")
    return int(t.shape[0]), int(t.shape[1]), int(t.stride(1))


def sam_attention(q, k, v, num_heads, scale=None, out=None):
    """softmax(q k^T scale) v per head for q [B, Nq, C], k, v [B, Nk, C] (row-strided views allowed) with min(Nq, Nk) <= 16 and
    C / num_heads in (16, 32): sgv3d_sam_attention.  Returns [B, Nq, C]."""
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.SGV3DError(f"sam_attention: {name} must be a tensor on the GPU (there is no CPU fallback)")
        if t.requires_grad and torch.is_grad_enabled():
            raise _lib.SGV3DError("sam_attention is inference only: an input requires grad and there is no backward")
        if t.dtype != torch.float32:
            raise _lib.SGV3DError(f"sam_attention: float32 {name} expected, got {t.dtype}")
    b, nq, q_ld = _rows(q, "q")
    bk, nk, k_ld = _rows(k, "k")
    bv, nv, v_ld = _rows(v, "v")
    c = int(q.shape[2])
    if (bk, bv) != (b, b) or nv != nk or int(k.shape[2]) != c or int(v.shape[2]) != c or c % int(num_heads):
        raise _lib.SGV3DError(f"sam_attention: shapes q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)}, heads {num_heads}")
    hd = c // int(num_heads)
    if out is None:
        out = torch.empty(b, nq, c, dtype=torch.float32, device=q.device)
    _, _, o_ld = _rows(out, "out")
    d = _lib.SamAttnDesc(b, nq, nk, int(num_heads), hd, q_ld, k_ld, v_ld, o_ld, float(hd ** -0.5 if scale is None else scale))
    lib = _lib.load()
    need = int(lib.sgv3d_sam_attention_workspace_bytes(ctypes.byref(d)))
    ws = torch.empty(need, dtype=torch.uint8, device=q.device) if need else None
    with torch.cuda.device(q.device):
        rc = lib.sgv3d_sam_attention(ctypes.byref(d), q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), _lib.ptr(ws), need,
                                     _lib.stream_handle(q.device))
    _lib.check(rc, "sgv3d_sam_attention")
    return out


def prompt_tokens(boxes, input_image_size, gauss, corner0, corner1, iou_token, mask_tokens):
    """boxes f32 [B, 4] -> the decoder's tokens [B, 7, dim] (sgv3d_sam_prompt_tokens)."""
    require_f32(boxes, "prompt_tokens")
    b, dim = int(boxes.shape[0]), int(gauss.shape[1]) * 2
    out = torch.empty(b, 7, dim, dtype=torch.float32, device=boxes.device)
    lib = _lib.load()
    with torch.cuda.device(boxes.device):
        rc = lib.sgv3d_sam_prompt_tokens(b, dim, int(input_image_size[0]), int(input_image_size[1]), boxes.data_ptr(), gauss.data_ptr(),
                                         corner0.data_ptr(), corner1.data_ptr(), iou_token.data_ptr(), mask_tokens.data_ptr(),
                                         out.data_ptr(), _lib.stream_handle(boxes.device))
    _lib.check(rc, "sgv3d_sam_prompt_tokens")
    return out


def dense_pe(gauss, h, w):
    """PositionEmbeddingRandom over an h x w grid as an NHWC map [1, h, w, dim] (sgv3d_sam_dense_pe)."""
    require_f32(gauss, "dense_pe")
    dim = int(gauss.shape[1]) * 2
    out = torch.empty(1, int(h), int(w), dim, dtype=torch.float32, device=gauss.device)
    lib = _lib.load()
    with torch.cuda.device(gauss.device):
        rc = lib.sgv3d_sam_dense_pe(int(h), int(w), dim, gauss.data_ptr(), out.data_ptr(), _lib.stream_handle(gauss.device))
    _lib.check(rc, "sgv3d_sam_dense_pe")
    return out


def gather_add(emb, frame_of_box, vec):
    """emb [F, h, w, C], frame_of_box i32 [B] (device, checked by the caller), vec [C] -> [B, h, w, C] = emb[frame] + vec."""
    require_f32(emb, "gather_add")
    f, h, w, c = (int(s) for s in emb.shape)
    b = int(frame_of_box.numel())
    out = torch.empty(b, h, w, c, dtype=torch.float32, device=emb.device)
    lib = _lib.load()
    with torch.cuda.device(emb.device):
        rc = lib.sgv3d_sam_gather_add(b, f, h * w, c, emb.data_ptr(), frame_of_box.data_ptr(), vec.data_ptr(), out.data_ptr(),
                                      _lib.stream_handle(emb.device))
    _lib.check(rc, "sgv3d_sam_gather_add")
    return out


def hyper_product(hyper, up):
    """hyper [B, n, C] (a view with dense [n, C] rows), up [B, H, W, C] -> [B, n, H, W] (sgv3d_sam_hyper_product)."""
    require_f32(up, "hyper_product")
    b, h, w, c = (int(s) for s in up.shape)
    n = int(hyper.shape[1])
    assert hyper.is_cuda and hyper.dtype == torch.float32 and hyper.stride(2) == 1 and hyper.stride(1) == c and int(hyper.shape[2]) == c
    out = torch.empty(b, n, h, w, dtype=torch.float32, device=up.device)
    lib = _lib.load()
    with torch.cuda.device(up.device):
        rc = lib.sgv3d_sam_hyper_product(b, h * w, c, n, int(hyper.stride(0)), hyper.data_ptr(), up.data_ptr(), out.data_ptr(),
                                         _lib.stream_handle(up.device))
    _lib.check(rc, "sgv3d_sam_hyper_product")
    return out


def mask_compose(mode, logits, size, pre_hw, out_hw, labels=None, frame_of_box=None, frames=1):
    """Low-res logits [B, low, low] -> COMPOSE_CLASS: u8 [frames, H, W]; COMPOSE_BOOL: bool [B, H, W]; COMPOSE_LOGIT: f32 [B, H, W]
    (sgv3d_sam_mask_compose).  ``logits`` may be None with COMPOSE_CLASS (no boxes): zeros."""
    lib = _lib.load()
    oh, ow = int(out_hw[0]), int(out_hw[1])
    if logits is None:
        if mode != COMPOSE_CLASS:
            raise _lib.SGV3DError("mask_compose: the per-box modes need logits")
        dev, b, low = labels.device, 0, 1
    else:
        require_f32(logits, "mask_compose")
        dev, b, low = logits.device, int(logits.shape[0]), int(logits.shape[-1])
        if logits.dim() != 3 or int(logits.shape[1]) != low:
            raise _lib.SGV3DError(f"mask_compose: square logits [B, low, low] expected, got {tuple(logits.shape)}")
    if mode == COMPOSE_CLASS:
        for t, name in ((labels, "labels"), (frame_of_box, "frame_of_box")):
            if t is None or not t.is_cuda or t.dtype != torch.int32 or t.numel() != b or not t.is_contiguous():
                raise _lib.SGV3DError(f"mask_compose: {name} must be a contiguous int32 device tensor with one entry per box")
        out = torch.empty(int(frames), oh, ow, dtype=torch.uint8, device=dev)
    elif mode == COMPOSE_BOOL:
        out = torch.empty(b, oh, ow, dtype=torch.uint8, device=dev)
    else:
        out = torch.empty(b, oh, ow, dtype=torch.float32, device=dev)
    need = int(lib.sgv3d_sam_mask_compose_workspace_bytes(oh, ow))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib.sgv3d_sam_mask_compose(int(mode), b, int(frames), low, int(size), int(pre_hw[0]), int(pre_hw[1]), oh, ow, _lib.ptr(logits),
                                        _lib.ptr(labels), _lib.ptr(frame_of_box), out.data_ptr(), ws.data_ptr(), need,
                                        _lib.stream_handle(dev))
    _lib.check(rc, "sgv3d_sam_mask_compose")
    return out.view(torch.bool) if mode == COMPOSE_BOOL else out


def mask_compose_host(mode, logits, size, pre_hw, out_hw, labels=None, frame_of_box=None, frames=1):
    """The host twin (sgv3d_sam_mask_compose_host) on numpy arrays: the same functions, pixel by pixel."""
    lib = _lib.load()
    oh, ow = int(out_hw[0]), int(out_hw[1])
    if logits is None:
        b, low, lp = 0, 1, None
    else:
        logits = np.ascontiguousarray(logits, np.float32)
        b, low, lp = int(logits.shape[0]), int(logits.shape[-1]), logits.ctypes.data
    lab = None if labels is None else np.ascontiguousarray(labels, np.int32)
    fob = None if frame_of_box is None else np.ascontiguousarray(frame_of_box, np.int32)
    shape = (int(frames), oh, ow) if mode == COMPOSE_CLASS else (b, oh, ow)
    out = np.empty(shape, np.float32 if mode == COMPOSE_LOGIT else np.uint8)
    rc = lib.sgv3d_sam_mask_compose_host(int(mode), b, int(frames), low, int(size), int(pre_hw[0]), int(pre_hw[1]), oh, ow, lp,
                                         None if lab is None else lab.ctypes.data, None if fob is None else fob.ctypes.data,
                                         out.ctypes.data)
    _lib.check(rc, "sgv3d_sam_mask_compose_host")
    return out.astype(bool) if mode == COMPOSE_BOOL else out


def resample_coeffs(filt, in_size, out_size):
    """Pillow's integer coefficients for one axis (host, sgv3d_resample_coeffs_filter): (bounds i32 [out, 2], coeffs i32 [out, k])."""
    lib = _lib.load()
    ks = ctypes.c_int(0)
    _lib.check(lib.sgv3d_resample_coeffs_filter(int(filt), int(in_size), int(out_size), None, None, ctypes.byref(ks)), "resample_coeffs_filter")
    bounds = np.zeros((int(out_size), 2), np.int32)
    coeffs = np.zeros((int(out_size), ks.value), np.int32)
    _lib.check(lib.sgv3d_resample_coeffs_filter(int(filt), int(in_size), int(out_size), bounds.ctypes.data, coeffs.ctypes.data,
                                                ctypes.byref(ks)), "resample_coeffs_filter")
    return bounds, coeffs


def resize_bilinear_u8_host(img, out_hw):
    """Pillow's BILINEAR Image.resize of a uint8 [H, W, C] array from the coefficient tables, in numpy (tests, small frames)."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]

    def axis_pass(a, n_in, n_out):            # along axis 1
        bounds, coeffs = resample_coeffs(FILTER_BILINEAR, n_in, n_out)
        out = np.empty((a.shape[0], n_out) + a.shape[2:], np.uint8)
        for o in range(n_out):
            x0, n = int(bounds[o, 0]), int(bounds[o, 1])
            acc = (a[:, x0:x0 + n].astype(np.int64) * coeffs[o, :n].reshape((1, n) + (1,) * (a.ndim - 2))).sum(1) + (1 << 21)
            out[:, o] = np.clip(acc >> 22, 0, 255)
        return out

    t = axis_pass(img, w, int(out_hw[1])) if int(out_hw[1]) != w else img
    if int(out_hw[0]) != h:
        t = axis_pass(t.swapaxes(0, 1), h, int(out_hw[0])).swapaxes(0, 1)
    return np.ascontiguousarray(t)


_TABLES = {}


def resize_bilinear_u8(frames, out_hw, swap_rb=False):
    """uint8 device frames [F, H, W, 3] -> Pillow's BILINEAR resize to ``out_hw`` as f32 [F, 3, oh, ow] holding the u8 values
    (sgv3d_resize_u8_filter): what torchvision's resize(to_pil_image(image), ...) gives, bit for bit."""
    if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
        raise _lib.SGV3DError("resize_bilinear_u8: the frames must be a tensor on the GPU (there is no CPU fallback)")
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3 or not frames.is_contiguous():
        raise _lib.SGV3DError(f"resize_bilinear_u8: contiguous uint8 [F, H, W, 3] frames expected, got {frames.dtype} {tuple(frames.shape)}")
    f, h, w, _ = (int(s) for s in frames.shape)
    oh, ow = int(out_hw[0]), int(out_hw[1])
    key = (h, w, oh, ow, str(frames.device))
    tab = _TABLES.get(key)
    if tab is None:
        xb, xc = resample_coeffs(FILTER_BILINEAR, w, ow)
        yb, yc = resample_coeffs(FILTER_BILINEAR, h, oh)
        tab = tuple(torch.from_numpy(a).to(frames.device) for a in (xb, xc, yb, yc)) + (xc.shape[1], yc.shape[1])
        _TABLES[key] = tab
    xb, xc, yb, yc, xk, yk = tab
    tmp = torch.empty(f, h, ow, 3, dtype=torch.uint8, device=frames.device)
    out = torch.empty(f, 3, oh, ow, dtype=torch.float32, device=frames.device)
    lib = _lib.load()
    with torch.cuda.device(frames.device):
        rc = lib.sgv3d_resize_u8_filter(f, h, w, oh, ow, xb.data_ptr(), xc.data_ptr(), xk, yb.data_ptr(), yc.data_ptr(), yk,
                                        1 if swap_rb else 0, frames.data_ptr(), tmp.data_ptr(), out.data_ptr(),
                                        _lib.stream_handle(frames.device))
    _lib.check(rc, "sgv3d_resize_u8_filter")
    return out
