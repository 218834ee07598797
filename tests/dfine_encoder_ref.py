"""Restatements for the temporal-encoder tests (dfine.self_attention / add_layer_norm / relu_dropout / encoder_layer_forward).

* torch expressions of the three ops and of the post-norm nn.TransformerEncoderLayer that take EXPLICIT keep-masks (bool, True =
  kept; None = no dropout) and run in any dtype on any device: float64 on the CPU is the reference of every numeric test, fp32 on
  the GPU is the baseline the kernels' error is measured against.
* the dropout keep-mask of the kernels in numpy: Philox4x32-10, element e of a site = word e % 4 of the block with counter
  (e // 4 low word, e // 4 high word, site, 0) and key (seed low word, seed high word), kept when word >= floor(float32(p) * 2^32).
"""
import math

import numpy as np
import torch

HEAD_DIM = 32
SITE_ATTN, SITE_ATTN_OUT, SITE_FFN, SITE_FFN_OUT = 0, 1, 2, 3

# ---- Philox4x32-10 ---------------------------------------------------------------------------------------------------------------
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two 32-bit ints -> four uint64 arrays holding the 32-bit result words"""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & _LO for x in counter]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = c[0] * _M0, c[2] * _M1          # 32 x 32 -> 64 bits, exact in uint64
        hi0, lo0, hi1, lo1 = p0 >> _S32, p0 & _LO, p1 >> _S32, p1 & _LO
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c


def keep_threshold(p) -> int:
    return int(float(np.float32(p)) * 4294967296.0)


def keep_mask(seed: int, site: int, shape, p) -> np.ndarray:
    """the bool keep-mask of a tensor of `shape` at dropout site `site`"""
    n = int(np.prod(shape))
    groups = np.arange((n + 3) // 4, dtype=np.uint64)
    zeros = np.zeros_like(groups)
    words = philox4x32_10((groups & _LO, groups >> _S32, zeros + np.uint64(site), zeros), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    flat = np.stack(words, axis=1).reshape(-1)[:n]
    return (flat >= np.uint64(keep_threshold(p))).reshape(shape)


def drop_scale(p) -> float:
    """1 / (1 - p) as the kernels form it: p rounded to float32 first"""
    return 1.0 / (1.0 - float(np.float32(p)))


# ---- the three ops and the layer in torch ops ----------------------------------------------------------------------------------
def _dropout(t, mask, p):
    if mask is None:
        return t
    return torch.where(mask.to(t.device), t * drop_scale(p), torch.zeros_like(t))


def self_attention(qkv, n_heads, mask=None, p=0.0):
    """qkv (B, S, 3 D) -> (B, S, D); mask (B, H, S, S) on the probabilities"""
    B, S, D3 = qkv.shape
    D = D3 // 3
    q, k, v = (t.reshape(B, S, n_heads, D // n_heads).transpose(1, 2) for t in qkv.split(D, dim=-1))
    prob = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(D // n_heads), dim=-1)
    return (_dropout(prob, mask, p) @ v).transpose(1, 2).reshape(B, S, D)


def add_layer_norm(x, y, weight, bias, eps, mask=None, p=0.0):
    return torch.nn.functional.layer_norm(x + _dropout(y, mask, p), (x.shape[-1],), weight, bias, eps)


def relu_dropout(h, mask=None, p=0.0):
    return _dropout(torch.relu(h), mask, p)


PARAM_NAMES = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
               "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight",
               "norm2.bias")


def layer_params(layer):
    """the 12 parameters of an nn.TransformerEncoderLayer as a dict under their state-dict names"""
    named = dict(layer.named_parameters())
    return {n: named[n] for n in PARAM_NAMES}


def encoder_layer(x, P, n_heads, eps=1e-5, masks=None, p=0.0):
    """the post-norm layer on a dict P of its 12 parameters; masks: None or the four keep-masks by site"""
    F = torch.nn.functional
    m = masks or {}
    a = self_attention(F.linear(x, P["self_attn.in_proj_weight"], P["self_attn.in_proj_bias"]), n_heads, m.get(SITE_ATTN), p)
    y = F.linear(a, P["self_attn.out_proj.weight"], P["self_attn.out_proj.bias"])
    x = add_layer_norm(x, y, P["norm1.weight"], P["norm1.bias"], eps, m.get(SITE_ATTN_OUT), p)
    h = relu_dropout(F.linear(x, P["linear1.weight"], P["linear1.bias"]), m.get(SITE_FFN), p)
    y = F.linear(h, P["linear2.weight"], P["linear2.bias"])
    return add_layer_norm(x, y, P["norm2.weight"], P["norm2.bias"], eps, m.get(SITE_FFN_OUT), p)


def encoder(x, layers, n_heads, eps=1e-5):
    for P in layers:
        x = encoder_layer(x, P, n_heads, eps)
    return x


def make_encoder(init: str, seed: int, d_model=256, nhead=8, ff=1024, dropout=0.0, num_layers=4):
    """the trainers' temporal encoder; init "tiny" = their normal(0, 1e-3) weights and zero biases, "default" = torch's own"""
    with torch.random.fork_rng():   # the global generator is left as it was
        torch.manual_seed(seed)
        layer = torch.nn.TransformerEncoderLayer(d_model=d_model, nhead=nhead, dim_feedforward=ff, dropout=dropout, batch_first=True)
        enc = torch.nn.TransformerEncoder(layer, num_layers=num_layers)   # deep copies: torch's default gives four equal layers
        if init == "tiny":
            # in_proj_weight is a bare Parameter that the trainers' isinstance(nn.Linear) loop does not reach: torch's xavier stays
            for m in enc.modules():
                if isinstance(m, torch.nn.Linear):
                    torch.nn.init.normal_(m.weight, mean=0.0, std=1e-3)
                    if m.bias is not None:
                        torch.nn.init.zeros_(m.bias)
                elif isinstance(m, torch.nn.LayerNorm):
                    torch.nn.init.ones_(m.weight)
                    torch.nn.init.zeros_(m.bias)
    return enc
