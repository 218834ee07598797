"""Gradient reference for the D-FINE ops (helper, torch on the CPU; not a test module).

The published structure of transformers' modeling_d_fine.py restated with differentiable torch ops, so that autograd
through it -- in float64 -- is the reference the HIP backward kernels are held to:
``multi_scale_deformable_attention_v2`` (:150-221) as one ``F.grid_sample`` per level ("default": bilinear, zeros
padding, align_corners=False) or an index gather ("discrete"); the softmax + sampling-location step of
``DFineMultiscaleDeformableAttention.forward`` (:268-296, 4-d reference points); ``DFineIntegral`` + ``distance2bbox``
(+ clamp).  tests/test_dfine_grad_host.py checks the forward of each against tests/golden/dfine_golden.npz and runs
torch.autograd.gradcheck on it.
"""
import torch
import torch.nn.functional as F


def msda(value, shapes, loc, attn, num_points_list, method="default"):
    """value (B, S, H, D); loc (B, Q, H, P, 2) or (B, Q, H, 1, P, 2); attn (B, Q, H, P) -> (B, Q, H * D)"""
    B, S, H, D = value.shape
    loc = loc.reshape(loc.shape[0], loc.shape[1], loc.shape[2], -1, 2)
    Q, P = loc.shape[1], loc.shape[3]
    v = value.permute(0, 2, 3, 1).flatten(0, 1)                              # (B * H, D, S)
    vals = v.split([h * w for h, w in shapes], dim=-1)
    locs = loc.permute(0, 2, 1, 3, 4).flatten(0, 1).split(list(num_points_list), dim=-2)   # (B * H, Q, n, 2) per level
    sampled = []
    for (h, w), val, lc in zip(shapes, vals, locs):
        val = val.reshape(B * H, D, h, w)
        if method == "default":
            sampled.append(F.grid_sample(val, 2 * lc - 1, mode="bilinear", padding_mode="zeros", align_corners=False))
        elif method == "discrete":
            # (loc * (w, h) + 0.5).to(int64), clamped per axis: no gradient reaches the locations.  The pixel is chosen in
            # float32 whatever dtype the gradients run in, so that a float64 run selects the pixels the op selects.
            xy = (lc.detach().to(torch.float32) * torch.tensor([w, h], dtype=torch.float32) + 0.5).to(torch.int64)
            x, y = xy[..., 0].clamp(0, w - 1), xy[..., 1].clamp(0, h - 1)
            idx = (y * w + x).reshape(B * H, 1, -1).expand(-1, D, -1)
            sampled.append(val.flatten(2).gather(2, idx).reshape(B * H, D, Q, -1))
        else:
            raise ValueError(method)
    a = attn.permute(0, 2, 1, 3).reshape(B * H, 1, Q, P)
    out = (torch.cat(sampled, dim=-1) * a).sum(-1)                           # (B * H, D, Q)
    return out.reshape(B, H * D, Q).permute(0, 2, 1)


def module_locations(ref, offsets, logits, num_points_list, offset_scale):
    """ref (B, Q, 4); offsets (B, Q, H, P, 2); logits (B, Q, H, P) -> sampling locations (B, Q, H, P, 2), weights"""
    attn = torch.softmax(logits, dim=-1)
    nscale = torch.tensor([1.0 / n for n in num_points_list for _ in range(n)], dtype=offsets.dtype).reshape(1, 1, 1, -1, 1)
    offset = offsets * nscale * ref[:, :, None, None, 2:] * offset_scale
    return ref[:, :, None, None, :2] + offset, attn


def module(value, shapes, ref, offsets, logits, num_points_list, offset_scale):
    loc, attn = module_locations(ref, offsets, logits, num_points_list, offset_scale)
    return msda(value, shapes, loc, attn, num_points_list, "default")


def deformable_attention(hidden, ref, enc, shapes, w_off, b_off, w_att, b_att, num_points_list, n_heads, offset_scale):
    """the two linear layers + `module`; enc (B, S, d), hidden (B, Q, d), ref (B, Q, 4)"""
    B, Q, d = hidden.shape
    P = sum(num_points_list)
    off = F.linear(hidden, w_off, b_off).reshape(B, Q, n_heads, P, 2)
    logit = F.linear(hidden, w_att, b_att).reshape(B, Q, n_heads, P)
    return module(enc.reshape(B, -1, n_heads, d // n_heads), shapes, ref, off, logit, num_points_list, offset_scale)


def decode_boxes(pred_corners, project, points, reg_scale, clamp01=False):
    """integral -> distance2bbox [-> clamp(0, 1)]; pred_corners (..., 4 * bins1), points (..., 4) -> (..., 4)"""
    nb1 = project.numel()
    p = torch.softmax(pred_corners.reshape(-1, nb1), dim=1)
    dist = F.linear(p, project.reshape(1, -1)).reshape(points.shape)
    rs = abs(reg_scale)
    x0 = points[..., 0] - (0.5 * rs + dist[..., 0]) * (points[..., 2] / rs)
    y0 = points[..., 1] - (0.5 * rs + dist[..., 1]) * (points[..., 3] / rs)
    x1 = points[..., 0] + (0.5 * rs + dist[..., 2]) * (points[..., 2] / rs)
    y1 = points[..., 1] + (0.5 * rs + dist[..., 3]) * (points[..., 3] / rs)
    boxes = torch.stack([(x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0], -1)
    return boxes.clamp(0, 1) if clamp01 else boxes


def grads(fn, inputs, grad_out, dtype):
    """inputs: dict name -> CPU tensor.  Runs fn(**inputs as `dtype` leaves) and returns (output, {name: gradient})."""
    leaves = {k: v.detach().to(dtype).requires_grad_(True) for k, v in inputs.items()}
    out = fn(**leaves)
    g = torch.autograd.grad(out, list(leaves.values()), grad_out.to(dtype), allow_unused=True)
    return out.detach(), {k: (torch.zeros_like(v) if gi is None else gi) for (k, v), gi in zip(leaves.items(), g)}


def ragged_case(D=32, seed=3):
    """Levels of one pixel, a 1 x 7 strip and 6 x 3; locations in [-0.3, 1.3], so some corners are outside the map; batch
    element 1 sits entirely at 7.0 (far outside: "default" gives it no gradient at all)."""
    g = torch.Generator().manual_seed(seed)
    shapes, pts = [(1, 1), (1, 7), (6, 3)], [1, 2, 5]
    B, Q, H = 3, 5, 2
    value = torch.randn(B, sum(h * w for h, w in shapes), H, D, generator=g)
    loc = torch.rand(B, Q, H, 8, 2, generator=g) * 1.6 - 0.3
    loc[1] = 7.0
    attn = torch.rand(B, Q, H, 8, generator=g)
    return shapes, pts, value, loc, attn
