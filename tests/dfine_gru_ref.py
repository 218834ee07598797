"""A numpy / float64 restatement of the one-layer GRU recurrence the kernels of csrc/dfine_gru.hip run, and of its gradient.

Shapes as in dfine.gru_recurrence: gi (B, S, D * 3H) are the input-side pre-activations of every step, gate order r, z, n, with
direction 1 (which walks the sequence from its end) in the second half of the last axis; w_hh (D, 3H, H); b_hh (D, 3H);
h0 (D, B, H) or None.  forward returns out (B, S, D * H), h_n (D, B, H) and what backward needs; backward returns the gradients
of the four inputs for upstream gradients on out and h_n."""
import numpy as np


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _steps(S, d):
    return range(S) if d == 0 else range(S - 1, -1, -1)


def forward(gi, w_hh, b_hh, h0=None):
    gi, w_hh, b_hh = (np.asarray(t, np.float64) for t in (gi, w_hh, b_hh))
    B, S, _ = gi.shape
    D, H3, H = w_hh.shape
    out = np.zeros((B, S, D * H))
    h_n = np.zeros((D, B, H))
    gates = np.zeros((D, S, 5, B, H))   # r, z, n, a_n and the state the step started from
    for d in range(D):
        h = np.zeros((B, H)) if h0 is None else np.asarray(h0, np.float64)[d].copy()
        for t in _steps(S, d):
            g = gi[:, t, d * H3:(d + 1) * H3]
            a = h @ w_hh[d].T + b_hh[d]
            r = _sigmoid(g[:, :H] + a[:, :H])
            z = _sigmoid(g[:, H:2 * H] + a[:, H:2 * H])
            n = np.tanh(g[:, 2 * H:] + r * a[:, 2 * H:])
            gates[d, t] = r, z, n, a[:, 2 * H:], h
            h = (1.0 - z) * n + z * h
            out[:, t, d * H:(d + 1) * H] = h
        h_n[d] = h
    return out, h_n, gates


def backward(grad_out, grad_h_n, w_hh, gates):
    """-> grad_gi (B, S, D * 3H), grad_w_hh (D, 3H, H), grad_b_hh (D, 3H), grad_h0 (D, B, H); grad_h_n may be None"""
    w_hh = np.asarray(w_hh, np.float64)
    grad_out = np.asarray(grad_out, np.float64)
    D, H3, H = w_hh.shape
    B, S, _ = grad_out.shape
    grad_gi = np.zeros((B, S, D * H3))
    grad_w = np.zeros((D, H3, H))
    grad_b = np.zeros((D, H3))
    grad_h0 = np.zeros((D, B, H))
    for d in range(D):
        dh = np.zeros((B, H)) if grad_h_n is None else np.asarray(grad_h_n, np.float64)[d].copy()
        for t in reversed(list(_steps(S, d))):
            r, z, n, a_n, h_prev = gates[d, t]
            dh = dh + grad_out[:, t, d * H:(d + 1) * H]
            d_n = dh * (1.0 - z) * (1.0 - n * n)          # through tanh
            d_z = dh * (h_prev - n) * z * (1.0 - z)       # through the update gate's sigmoid
            d_r = d_n * a_n * r * (1.0 - r)               # through the reset gate's sigmoid
            grad_gi[:, t, d * H3:(d + 1) * H3] = np.concatenate([d_r, d_z, d_n], axis=1)
            d_a = np.concatenate([d_r, d_z, d_n * r], axis=1)
            grad_w[d] += d_a.T @ h_prev
            grad_b[d] += d_a.sum(axis=0)
            dh = dh * z + d_a @ w_hh[d]
        grad_h0[d] = dh
    return grad_gi, grad_w, grad_b, grad_h0
