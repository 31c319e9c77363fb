"""The adjoints of tests/vit_ref.py written out by hand, without autograd: the attention backward of the header
(include/sgv3d_hip.h, sgv3d_vit_attention_backward) formula by formula, LayerNorm, GELU and the bilinear resize, and the whole
encoder's parameter gradients chained from them.  Runs in the dtype of its inputs: float64 on the CPU is the yardstick of the
tests, float32 on the CPU sets their bars (4 x its error, the summation orders differ).

The keyword switches of ``attention_backward`` are the four misreadings the gradient fixture guards against (its maker asserts
that each moves a named gradient by more than 100 x its bar):
  pad_bias=False        the padding slots' dk / dv left out of dpad_qkv (so out of qkv.bias.grad)
  rel_in_dq=False       the relative-position terms left out of dq
  rel_scaled_q=True     the scaled q in dRh / dRw
  pad_queries=True      padding slots counted as queries (they take the cotangent of the nearest map pixel)
"""
import math

import torch

import vit_ref as V


def to_byte_planes(a):
    """float32 array -> uint8 [4, n]: byte k of every value side by side (what tests/golden/sam_encoder_grad*.npz store)."""
    import numpy as np
    return np.ascontiguousarray(np.ascontiguousarray(a, dtype='<f4').reshape(-1).view(np.uint8).reshape(-1, 4).T)


class open_fixture:
    """tests/golden/sam_encoder_grad.npz (``embed``: sam_encoder_grad_embed.npz) and its remainder file ..._rem.npz read as one."""

    def __init__(self, golden_dir, embed=False):
        import os
        import numpy as np
        stem = os.path.join(golden_dir, 'sam_encoder_grad_embed' if embed else 'sam_encoder_grad')
        self._parts = [np.load(stem + '.npz'), np.load(stem + '_rem.npz')]
        self.files = [k for part in self._parts for k in part.files]

    def __getitem__(self, key):
        for part in self._parts:
            if key in part.files:
                return part[key]
        raise KeyError(key)


def fixture_grad(fx, name):
    """The float64 gradient of parameter ``name`` in an ``open_fixture``: stored as float64, or, for tensors of 1024 elements or
    more, as a float32 head plus a float32 remainder (see the maker)."""
    import numpy as np
    if f'grad/{name}' in fx.files:
        return torch.from_numpy(fx[f'grad/{name}']).double()
    shape = tuple(fx[f'grad_shape/{name}'])
    part = lambda key: np.ascontiguousarray(fx[key].T).view('<f4').reshape(shape).astype(np.float64)
    return torch.from_numpy(part(f'grad_planes/{name}') + part(f'grad_rem_planes/{name}'))


def _windows(x, num_heads, window, replicate=False):
    """[B, H, W, C] -> [B, ny, nx, heads, T, hd] of the map padded to whole windows with zeros (or edge-replicated)."""
    b, h, w, c = x.shape
    wh, ww = window
    hd = c // num_heads
    ny, nx = -(-h // wh), -(-w // ww)
    if replicate:
        iy = torch.clamp(torch.arange(ny * wh), max=h - 1)
        ix = torch.clamp(torch.arange(nx * ww), max=w - 1)
        full = x[:, iy][:, :, ix]
    else:
        full = x.new_zeros(b, ny * wh, nx * ww, c)
        full[:, :h, :w] = x
    return full.reshape(b, ny, wh, nx, ww, num_heads, hd).permute(0, 1, 3, 5, 2, 4, 6).reshape(b, ny, nx, num_heads, wh * ww, hd)


def attention_forward(qkv, num_heads, window, pad_qkv=None, rel_pos_h=None, rel_pos_w=None):
    """-> out [B, H, W, C], lse [B, heads, H, W]."""
    b, h, w, _ = qkv.shape
    q, k, v, _ = V.split_windows(qkv, num_heads, window, pad_qkv)
    s = V.window_logits(q, k, window, rel_pos_h, rel_pos_w)
    lse = torch.logsumexp(s, -1)
    o = torch.exp(s - lse.unsqueeze(-1)) @ v
    lse_map = V.merge_windows(lse.unsqueeze(-1), window, h, w).permute(0, 3, 1, 2).contiguous()
    return V.merge_windows(o, window, h, w), lse_map


def attention_backward(qkv, num_heads, window, pad_qkv, rel_pos_h, rel_pos_w, dout, pad_bias=True, rel_in_dq=True,
                       rel_scaled_q=False, pad_queries=False):
    """-> dqkv [B, H, W, 3 C], dpad_qkv [3 C], drel_pos_h, drel_pos_w (None without tables)."""
    b, h, w, c3 = qkv.shape
    wh, ww = window
    c = c3 // 3
    hd = c // num_heads
    scale = hd ** -0.5
    q, k, v, real = V.split_windows(qkv, num_heads, window, pad_qkv)
    s = V.window_logits(q, k, window, rel_pos_h, rel_pos_w)
    lse = torch.logsumexp(s, -1, keepdim=True)
    p = torch.exp(s - lse)                                   # P_ij
    o = p @ v
    do = _windows(dout, num_heads, window, replicate=pad_queries)     # zero rows for the padding slots: never a query
    delta = (do * o).sum(-1, keepdim=True)                   # delta_i
    dp = do @ v.transpose(-1, -2)                            # dP_ij
    ds = p * (dp - delta)                                    # dS_ij
    dv = p.transpose(-1, -2) @ do
    dk = scale * (ds.transpose(-1, -2) @ q)
    dq = scale * (ds @ k)
    drh = drw = None
    if rel_pos_h is not None:
        lead = ds.shape[:-2]
        ds5 = ds.reshape(*lead, wh, ww, wh, ww)
        a_h, a_w = ds5.sum(-1), ds5.sum(-2)                  # [..., qh, qw, kh], [..., qh, qw, kw]
        ih, iw = torch.arange(wh), torch.arange(ww)
        idx_h = ih[:, None] - ih[None, :] + wh - 1           # [qh, kh]
        idx_w = iw[:, None] - iw[None, :] + ww - 1
        rh, rw = rel_pos_h.to(qkv.dtype)[idx_h], rel_pos_w.to(qkv.dtype)[idx_w]       # [qh, kh, hd], [qw, kw, hd]
        if rel_in_dq:
            dq = dq + (torch.einsum('...hwa,had->...hwd', a_h, rh) + torch.einsum('...hwb,wbd->...hwd', a_w, rw)).reshape(dq.shape)
        qq = (q * scale if rel_scaled_q else q).reshape(*lead, wh, ww, hd)
        n = a_h.numel() // (wh * ww * wh)
        gh = torch.einsum('nhwa,nhwd->had', a_h.reshape(n, wh, ww, wh), qq.reshape(n, wh, ww, hd))
        gw = torch.einsum('nhwb,nhwd->wbd', a_w.reshape(n, wh, ww, ww), qq.reshape(n, wh, ww, hd))
        drh = torch.zeros_like(rel_pos_h, dtype=qkv.dtype).index_add_(0, idx_h.reshape(-1), gh.reshape(-1, hd))
        drw = torch.zeros_like(rel_pos_w, dtype=qkv.dtype).index_add_(0, idx_w.reshape(-1), gw.reshape(-1, hd))
    dqkv = torch.cat([V.merge_windows(t, window, h, w) for t in (dq, dk, dv)], -1)
    dpad = qkv.new_zeros(3, num_heads, hd)
    if pad_bias:
        m = (~real).to(qkv.dtype)[None, :, :, None, :, None]         # [1, ny, nx, 1, T, 1]
        dpad[1] = (dk * m).sum((0, 1, 2, 4))
        dpad[2] = (dv * m).sum((0, 1, 2, 4))
    return dqkv, dpad.reshape(-1), drh, drw


def layernorm_backward(x, weight, eps, dy):
    """-> dx, dweight, dbias of vit_ref.layernorm over the last dimension."""
    mu = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + eps)
    xh = (x - mu) * rstd
    g = dy * weight
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    red = tuple(range(x.dim() - 1))
    return dx, (dy * xh).sum(red), dy.sum(red)


def gelu_backward(x, dy):
    """dy (Phi(x) + x phi(x))."""
    cdf = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return dy * (cdf + x * pdf)


def _tap_matrix(n_in, n_out, dtype):
    """[n_out, n_in]: the weight with which output o reads input i."""
    i0, i1, lam = V._taps(n_in, n_out, dtype, 'cpu')
    m = torch.zeros(n_out, n_in, dtype=dtype)
    o = torch.arange(n_out)
    m.index_put_((o, i0), 1 - lam, accumulate=True)
    m.index_put_((o, i1), lam, accumulate=True)
    return m


def resize_bilinear_backward(dy, in_hw, crop):
    """dy [B, oh, ow, C] -> dx [B, h, w, C]: zero outside the (clamped) crop."""
    b, oh, ow, c = dy.shape
    h, w = in_hw
    ch, cw = min(crop[0], h), min(crop[1], w)
    wy, wx = _tap_matrix(ch, oh, dy.dtype), _tap_matrix(cw, ow, dy.dtype)
    dx = dy.new_zeros(b, h, w, c)
    dx[:, :ch, :cw] = torch.einsum('oi,pj,bopc->bijc', wy, wx, dy)
    return dx


def _linear_backward(x, weight, dy):
    """y = x W^T + b on [..., cin] -> dx, dW, db."""
    x2, d2 = x.reshape(-1, x.shape[-1]), dy.reshape(-1, dy.shape[-1])
    return dy @ weight, d2.t() @ x2, d2.sum(0)


def encoder_backward(wts, cfg, img, cot, embed=False, **attn_kw):
    """Parameter gradients of sum(out * cot) by hand.  ``embed=False``: out = vit_ref.encoder_forward [B, out_chans, oh, ow];
    ``embed=True``: out = the NHWC neck output [B, H, W, out_chans] that ImageEncoderViT.embed returns.  -> {name: gradient}."""
    F = torch.nn.functional
    dt = img.dtype
    g = lambda name: wts[name].to(dt)
    mean = torch.tensor([123.675, 116.28, 103.53], dtype=torch.float32).to(dt)
    std = torch.tensor([58.395, 57.12, 57.375], dtype=torch.float32).to(dt)
    ps = cfg['patch_size']
    x0 = V.preprocess(img, mean, std, cfg['img_size'])
    b = x0.shape[0]
    hh = ww = cfg['img_size'] // ps
    patches = x0.reshape(b, 3, hh, ps, ww, ps).permute(0, 2, 4, 1, 3, 5).reshape(b, hh, ww, 3 * ps * ps)
    wpe = g('patch_embed.proj.weight').reshape(-1, 3 * ps * ps)
    x = patches @ wpe.t() + g('patch_embed.proj.bias') + g('pos_embed')
    tape = []
    for i in range(cfg['depth']):
        pre = f'blocks.{i}.'
        ws = 0 if i in cfg['global_attn_indexes'] else cfg['window_size']
        win = (ws, ws) if ws else (hh, ww)
        t = dict(x_in=x, win=win)
        t['y1'] = V.layernorm(x, g(pre + 'norm1.weight'), g(pre + 'norm1.bias'), cfg['eps'])
        t['qkv'] = t['y1'] @ g(pre + 'attn.qkv.weight').t() + g(pre + 'attn.qkv.bias')
        t['a'] = V.attention(t['qkv'], cfg['num_heads'], win, g(pre + 'attn.qkv.bias'), g(pre + 'attn.rel_pos_h'), g(pre + 'attn.rel_pos_w'))
        x = x + (t['a'] @ g(pre + 'attn.proj.weight').t() + g(pre + 'attn.proj.bias'))
        t['x_mid'] = x
        t['y2'] = V.layernorm(x, g(pre + 'norm2.weight'), g(pre + 'norm2.bias'), cfg['eps'])
        t['h'] = t['y2'] @ g(pre + 'mlp.lin1.weight').t() + g(pre + 'mlp.lin1.bias')
        t['gh'] = V.gelu(t['h'])
        x = x + (t['gh'] @ g(pre + 'mlp.lin2.weight').t() + g(pre + 'mlp.lin2.bias'))
        tape.append(t)
    x_blocks = x
    w0 = g('neck.0.weight')
    n0 = x_blocks @ w0.reshape(w0.shape[0], -1).t()
    n1 = V.layernorm(n0, g('neck.1.weight'), g('neck.1.bias'), 1e-6)
    w2 = g('neck.2.weight')
    oc = w2.shape[0]
    cols = F.unfold(n1.permute(0, 3, 1, 2), 3, padding=1)                 # [B, C * 9, L]
    n2 = (w2.reshape(oc, -1) @ cols).transpose(1, 2).reshape(b, hh, ww, oc)
    grads = {}
    if embed:
        d = cot
    else:
        dd = cfg['downsample_factor']
        d = resize_bilinear_backward(cot.permute(0, 2, 3, 1), (hh, ww), (576 // dd, 1024 // dd))
    d, grads['neck.3.weight'], grads['neck.3.bias'] = layernorm_backward(n2, g('neck.3.weight'), 1e-6, d)
    d2 = d.reshape(b, hh * ww, oc).transpose(1, 2)                       # [B, oc, L]
    grads['neck.2.weight'] = torch.einsum('bol,bkl->ok', d2, cols).reshape(w2.shape)
    d = F.fold(w2.reshape(oc, -1).t() @ d2, (hh, ww), 3, padding=1).permute(0, 2, 3, 1)
    d, grads['neck.1.weight'], grads['neck.1.bias'] = layernorm_backward(n0, g('neck.1.weight'), 1e-6, d)
    d, dw, _ = _linear_backward(x_blocks, w0.reshape(w0.shape[0], -1), d)
    grads['neck.0.weight'] = dw.reshape(w0.shape)
    for i in reversed(range(cfg['depth'])):
        pre = f'blocks.{i}.'
        t = tape[i]
        dh, grads[pre + 'mlp.lin2.weight'], grads[pre + 'mlp.lin2.bias'] = _linear_backward(t['gh'], g(pre + 'mlp.lin2.weight'), d)
        dh = gelu_backward(t['h'], dh)
        dy2, grads[pre + 'mlp.lin1.weight'], grads[pre + 'mlp.lin1.bias'] = _linear_backward(t['y2'], g(pre + 'mlp.lin1.weight'), dh)
        dxm, grads[pre + 'norm2.weight'], grads[pre + 'norm2.bias'] = layernorm_backward(t['x_mid'], g(pre + 'norm2.weight'), cfg['eps'], dy2)
        d = d + dxm
        da, grads[pre + 'attn.proj.weight'], grads[pre + 'attn.proj.bias'] = _linear_backward(t['a'], g(pre + 'attn.proj.weight'), d)
        dqkv, dpad, grads[pre + 'attn.rel_pos_h'], grads[pre + 'attn.rel_pos_w'] = attention_backward(
            t['qkv'], cfg['num_heads'], t['win'], g(pre + 'attn.qkv.bias'), g(pre + 'attn.rel_pos_h'), g(pre + 'attn.rel_pos_w'), da, **attn_kw)
        dy1, grads[pre + 'attn.qkv.weight'], db = _linear_backward(t['y1'], g(pre + 'attn.qkv.weight'), dqkv)
        grads[pre + 'attn.qkv.bias'] = db + dpad
        dxi, grads[pre + 'norm1.weight'], grads[pre + 'norm1.bias'] = layernorm_backward(t['x_in'], g(pre + 'norm1.weight'), cfg['eps'], dy1)
        d = d + dxi
    grads['pos_embed'] = d.sum(0, keepdim=True)
    _, dw, grads['patch_embed.proj.bias'] = _linear_backward(patches, wpe, d)
    grads['patch_embed.proj.weight'] = dw.reshape(wts['patch_embed.proj.weight'].shape)
    return grads
