"""Restatement of SAM's ViT image encoder in plain torch, written from its description (not from the reference's file):
explicit padded windows, the qkv bias as the padding tokens, a relative-position bias built by index, hand-written
LayerNorm, erf GELU and bilinear taps.  It runs in the dtype and on the device of its inputs: float64 on the CPU is the
yardstick of the tests, float32 on the GPU is the baseline tools/vit_bench.py times.

The keyword switches of ``attention`` exist for the three misreadings the fixture guards against (its maker asserts
that each moves the output by more than 1e-2): padding tokens masked out, padding tokens as zeros, and the scaled q in
the relative-position terms.
"""
import math

import torch


def layernorm(x, weight, bias, eps):
    """Over the last dimension."""
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * weight + bias


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def preprocess(img, mean, std, size):
    """[B, 3, H, W] -> [B, 3, size, size]: normalise, THEN pad with zeros at the bottom and the right."""
    b, c, h, w = img.shape
    out = img.new_zeros(b, c, size, size)
    out[:, :, :h, :w] = (img - mean.reshape(1, 3, 1, 1)) / std.reshape(1, 3, 1, 1)
    return out


def _taps(n_in, n_out, dtype, device):
    o = torch.arange(n_out, dtype=dtype, device=device)
    src = torch.clamp((o + 0.5) * (n_in / n_out) - 0.5, min=0.0)
    i0 = torch.clamp(src.floor().long(), max=n_in - 1)
    i1 = torch.clamp(i0 + 1, max=n_in - 1)
    lam = src - i0.to(dtype)
    return i0, i1, lam


def resize_bilinear(x, crop, size):
    """NHWC: x[:, :crop_h, :crop_w] (clamped to the map), then bilinear with align_corners=False to ``size``."""
    x = x[:, :min(crop[0], x.shape[1]), :min(crop[1], x.shape[2])]
    y0, y1, ly = _taps(x.shape[1], size[0], x.dtype, x.device)
    x0, x1, lx = _taps(x.shape[2], size[1], x.dtype, x.device)
    ly, lx = ly.reshape(1, -1, 1, 1), lx.reshape(1, 1, -1, 1)
    top = x[:, y0][:, :, x0] * (1 - lx) + x[:, y0][:, :, x1] * lx
    bot = x[:, y1][:, :, x0] * (1 - lx) + x[:, y1][:, :, x1] * lx
    return top * (1 - ly) + bot * ly


def split_windows(qkv, num_heads, window, pad_qkv=None):
    """[B, H, W, 3 C] -> q, k, v [B, ny, nx, heads, T, hd] of the map padded to whole windows with ``pad_qkv`` tokens, and
    ``real`` [ny, nx, T]: which window slots hold a token of the map."""
    b, h, w, c3 = qkv.shape
    wh, ww = window
    hd = c3 // 3 // num_heads
    ny, nx = -(-h // wh), -(-w // ww)
    pad = qkv.new_zeros(c3) if pad_qkv is None else pad_qkv.to(qkv.dtype)
    full = pad.reshape(1, 1, 1, c3).repeat(b, ny * wh, nx * ww, 1)
    full[:, :h, :w] = qkv
    real = torch.zeros(ny * wh, nx * ww, dtype=torch.bool, device=qkv.device)
    real[:h, :w] = True
    x = full.reshape(b, ny, wh, nx, ww, 3, num_heads, hd).permute(5, 0, 1, 3, 6, 2, 4, 7).reshape(3, b, ny, nx, num_heads, wh * ww, hd)
    real = real.reshape(ny, wh, nx, ww).permute(0, 2, 1, 3).reshape(ny, nx, wh * ww)
    return x[0], x[1], x[2], real


def window_logits(q, k, window, rel_pos_h=None, rel_pos_w=None, rel_uses_scaled_q=False):
    """q, k [..., T, hd] of windows -> logits [..., T, T]: (q hd^-0.5) . k + q . R_h[qh - kh + wh - 1] + q . R_w[qw - kw + ww - 1]."""
    wh, ww = window
    hd = q.shape[-1]
    scale = hd ** -0.5
    logits = (q * scale) @ k.transpose(-1, -2)
    if rel_pos_h is not None:
        assert rel_pos_h.shape[0] == 2 * wh - 1 and rel_pos_w.shape[0] == 2 * ww - 1
        ih = torch.arange(wh, device=q.device)
        iw = torch.arange(ww, device=q.device)
        rh = rel_pos_h.to(q.dtype)[ih[:, None] - ih[None, :] + wh - 1]      # [qh, kh, hd]
        rw = rel_pos_w.to(q.dtype)[iw[:, None] - iw[None, :] + ww - 1]      # [qw, kw, hd]
        qq = (q * scale if rel_uses_scaled_q else q).reshape(*q.shape[:-2], wh, ww, hd)
        bh = (qq.unsqueeze(-2) * rh.reshape(wh, 1, wh, hd)).sum(-1)         # [..., qh, qw, kh]
        bw = (qq.unsqueeze(-2) * rw.reshape(1, ww, ww, hd)).sum(-1)         # [..., qh, qw, kw]
        logits = (logits.reshape(*q.shape[:-2], wh, ww, wh, ww) + bh.unsqueeze(-1) + bw.unsqueeze(-2)).reshape(logits.shape)
    return logits


def attention(qkv, num_heads, window, pad_qkv=None, rel_pos_h=None, rel_pos_w=None, pad_keys='token', rel_uses_scaled_q=False):
    """qkv [B, H, W, 3 C], last dimension ordered (3, heads, hd) -> [B, H, W, C]; ``window`` (wh, ww), global = (H, W)."""
    b, h, w, c3 = qkv.shape
    wh, ww = window
    c = c3 // 3
    if pad_keys == 'zero':
        pad_qkv = None
    q, k, v, real = split_windows(qkv, num_heads, window, pad_qkv)
    logits = window_logits(q, k, window, rel_pos_h, rel_pos_w, rel_uses_scaled_q)
    if pad_keys == 'masked':
        logits = logits.masked_fill(~real[None, :, :, None, None, :], float('-inf'))
    p = torch.softmax(logits, dim=-1)
    o = p @ v                                                                # [B, ny, nx, heads, T, hd]
    return merge_windows(o, window, h, w)


def merge_windows(o, window, h, w):
    """[B, ny, nx, heads, T, hd] of windows -> the map [B, h, w, heads * hd] (the padding rows and columns dropped)."""
    b, ny, nx, nh, _, hd = o.shape
    wh, ww = window
    o = o.reshape(b, ny, nx, nh, wh, ww, hd).permute(0, 1, 4, 2, 5, 3, 6).reshape(b, ny * wh, nx * ww, nh * hd)
    return o[:, :h, :w].contiguous()


def encoder_forward(wts, cfg, img, block_outputs=None, **attn_kw):
    """The whole encoder from a state dict ``wts`` (the reference's parameter names).  ``cfg``: img_size, patch_size, depth,
    num_heads, window_size, global_attn_indexes, eps, final_dim, downsample_factor.  Returns [B, out_chans, oh, ow];
    ``block_outputs`` (a list) receives every block's [B, H, W, C] output."""
    F = torch.nn.functional
    dt = img.dtype
    g = lambda name: wts[name].to(dt)
    # the reference keeps these as float32 buffers: the float64 run sees the float32-rounded values
    mean = torch.tensor([123.675, 116.28, 103.53], dtype=torch.float32, device=img.device).to(dt)
    std = torch.tensor([58.395, 57.12, 57.375], dtype=torch.float32, device=img.device).to(dt)
    x = preprocess(img, mean, std, cfg['img_size'])
    x = F.conv2d(x, g('patch_embed.proj.weight'), g('patch_embed.proj.bias'), stride=cfg['patch_size']).permute(0, 2, 3, 1)
    x = x + g('pos_embed')
    hh, ww = x.shape[1], x.shape[2]
    for i in range(cfg['depth']):
        pre = f'blocks.{i}.'
        ws = 0 if i in cfg['global_attn_indexes'] else cfg['window_size']
        y = layernorm(x, g(pre + 'norm1.weight'), g(pre + 'norm1.bias'), cfg['eps'])
        qkv = y @ g(pre + 'attn.qkv.weight').t() + g(pre + 'attn.qkv.bias')
        a = attention(qkv, cfg['num_heads'], (ws, ws) if ws else (hh, ww), g(pre + 'attn.qkv.bias'),
                      g(pre + 'attn.rel_pos_h'), g(pre + 'attn.rel_pos_w'), **attn_kw)
        x = x + (a @ g(pre + 'attn.proj.weight').t() + g(pre + 'attn.proj.bias'))
        y = layernorm(x, g(pre + 'norm2.weight'), g(pre + 'norm2.bias'), cfg['eps'])
        y = gelu(y @ g(pre + 'mlp.lin1.weight').t() + g(pre + 'mlp.lin1.bias'))
        x = x + (y @ g(pre + 'mlp.lin2.weight').t() + g(pre + 'mlp.lin2.bias'))
        if block_outputs is not None:
            block_outputs.append(x)
    x = F.conv2d(x.permute(0, 3, 1, 2), g('neck.0.weight')).permute(0, 2, 3, 1)
    x = layernorm(x, g('neck.1.weight'), g('neck.1.bias'), 1e-6)
    x = F.conv2d(x.permute(0, 3, 1, 2), g('neck.2.weight'), padding=1).permute(0, 2, 3, 1)
    x = layernorm(x, g('neck.3.weight'), g('neck.3.bias'), 1e-6)
    d = cfg['downsample_factor']
    x = resize_bilinear(x, (576 // d, 1024 // d), (cfg['final_dim'][0] // d, cfg['final_dim'][1] // d))
    return x.permute(0, 3, 1, 2)


FIXTURE_CFG = dict(img_size=96, patch_size=8, embed_dim=64, depth=2, num_heads=2, out_chans=32, window_size=5,
                   global_attn_indexes=[1], eps=1e-6, final_dim=(864, 1536), downsample_factor=64)
