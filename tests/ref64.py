"""The second judge of the op tests: plain binary64 restatements of the reference's operations (torch.nn.functional / numpy).

The C oracle (oracle/c) shares its fma chains with the kernels on purpose, so "engine == oracle" proves that two programs agree, not
that they compute a convolution.  Nothing here is canonical and nothing is shared with the oracle or the engine: the operations are
written from their definitions, evaluated in binary64, and compared through error bounds that are derived (dot_bound) or measured from
references alone (aten_tol), never from the code under test.  Inputs are the binary32 arrays of the tests, widened exactly.
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24          # unit roundoff of binary32


def _t(a, dtype=torch.float64):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


# ------------------------------------------------------------------------------------------------------------- convolutions
def conv1d(x, w, b=None, stride=1, pad=0, dil=1, groups=1, residual=None):
    """conv1d on x [B,Cin,T] with w [Cout,Cin/groups,K]; `residual` [B,Cout,Tout] is added after the bias."""
    y = F.conv1d(_t(x), _t(w), _t(b), stride=stride, padding=pad, dilation=dil, groups=groups)
    if residual is not None:
        y = y + _t(residual)
    return y.numpy()


def conv_transpose1d(x, w, b=None, stride=1, pad=0, out_pad=0):
    """conv_transpose1d on x [B,Cin,T] with w [Cin,Cout,K]."""
    return F.conv_transpose1d(_t(x), _t(w), _t(b), stride=stride, padding=pad, output_padding=out_pad).numpy()


def gamma(n):
    n = float(n)
    return n * U / (1.0 - n * U)


def dot_bound(n_terms, abs_dot):
    """Forward error bound of an n-term binary32 fma/add chain in any order: gamma(n) * sum |a_i b_i| (Higham, Accuracy and Stability of
    Numerical Algorithms, section 3.1).  `abs_dot` is that sum, evaluated in binary64 by running the same operation on absolute values."""
    return gamma(n_terms) * np.asarray(abs_dot, np.float64)


def _abs(a):
    return None if a is None else np.abs(np.asarray(a, np.float64))


def conv1d_bound(x, w, b=None, stride=1, pad=0, dil=1, groups=1, residual=None):
    """|binary32 conv1d - binary64 conv1d| <= this, element by element: reduction length + 1 (bias) + 1 (residual) terms."""
    n = (w.shape[1] * w.shape[2]) + 1 + (1 if residual is not None else 0)
    return dot_bound(n, conv1d(_abs(x), _abs(w), _abs(b), stride, pad, dil, groups, _abs(residual)))


def conv_transpose1d_bound(x, w, b=None, stride=1, pad=0, out_pad=0):
    """An output sample of a transposed convolution sums Cin * ceil(K / stride) products (the taps of its phase) and the bias."""
    n = w.shape[0] * (-(-w.shape[2] // stride)) + 1
    return dot_bound(n, conv_transpose1d(_abs(x), _abs(w), _abs(b), stride, pad, out_pad))


def dwconv_first_t(x, w, b=None, pad=0, dil=1):
    """What the engine's depthwise hook defines: y[b,c,t] = sum_k w[c,k] x[b,c,t + k dil - pad] + bias[c] for t in [0, T) over the
    zero-extended row.  Written as an explicit tap loop (not through F.conv1d) so that it shares nothing with conv1d above."""
    x = np.asarray(x, np.float64); w = np.asarray(w, np.float64).reshape(x.shape[1], -1)
    B, C, T = x.shape
    K = w.shape[1]
    right = max(0, (K - 1) * dil - pad)
    xp = np.pad(x, ((0, 0), (0, 0), (pad, right)))
    y = np.zeros((B, C, T), np.float64)
    for k in range(K):
        y += w[None, :, k, None] * xp[:, :, k * dil:k * dil + T]
    if b is not None:
        y += np.asarray(b, np.float64)[None, :, None]
    return y


def dwconv_first_t_bound(x, w, b=None, pad=0, dil=1):
    K = np.asarray(w).reshape(np.asarray(x).shape[1], -1).shape[1]
    return dot_bound(K + 1, dwconv_first_t(_abs(x), _abs(w), _abs(b), pad, dil))


# ------------------------------------------------------------------------------------------------------------- activations
def snake(x, alpha):
    """Snake1d.cs:52-63: x + sin^2(alpha x) / alpha with the true quotient; alpha == 0 -> x.  x [B,C,T], alpha [C]."""
    x = np.asarray(x, np.float64)
    a = np.asarray(alpha, np.float64).reshape(1, -1, 1)
    safe = np.where(a == 0.0, 1.0, a)
    return np.where(a == 0.0, x, x + np.sin(a * x) ** 2 / safe)


def tanh(x):
    return np.tanh(np.asarray(x, np.float64))


def elu(x):
    x = np.asarray(x, np.float64)
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0.0)))


def ulp32(y):
    """Spacing of binary32 at |y| (the unit the activation tables of tests/golden/op_error_bounds.json are in); denormal spacing below 2^-126."""
    a = np.abs(np.asarray(y, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))
    return 2.0 ** (e - 23)


# ------------------------------------------------------------------------------------------------------------- SNAC pieces
def layer_norm_ct(x, gamma_, beta, eps=1e-5, dtype=torch.float64):
    """LayerNorm over the channel axis of x [B,C,T] (LocalMHA.cs:85).  dtype=torch.float32 gives ATen's own binary32 answer."""
    C = x.shape[1]
    y = F.layer_norm(_t(x, dtype).transpose(1, 2), (C,), _t(gamma_, dtype), _t(beta, dtype), eps)
    return y.transpose(1, 2).contiguous().numpy()


def avg_pool(x, s):
    """avg_pool1d(s) over the last axis of x [rows,T] -> [rows, T // s] (the tail that does not fill a window is dropped)."""
    x = np.asarray(x, np.float64)
    Ts = x.shape[-1] // s
    return x[:, :Ts * s].reshape(x.shape[0], Ts, s).mean(axis=2)


def avg_pool_bound(x, s):
    """s - 1 additions and one division: gamma(s) * mean|x|."""
    return dot_bound(s, avg_pool(np.abs(np.asarray(x, np.float64)), s))


def rotary_inv_freq():
    """SinusoidalEmbedding.cs:44-47: 1 / 10000 ** (arange(0, 64, 2) / 64), binary32 as the checkpoints store it."""
    return (1.0 / (10000 ** (torch.arange(0, 64, 2).float() / 64))).numpy()


def local_attn(qkv, W, inv_freq=None, dtype=torch.float64):
    """LocalMHA.cs:84-113 without its projections: qkv [B,3C,T] (channel = part*C + head*64 + d) -> [B,C,T].  Heads of 64 features, windows
    of W steps, rotary embedding on q and k by the position inside the window (scale == 1), non-causal softmax(q k^T / 8) v per window."""
    B, C3, T = qkv.shape
    C, H, NW = C3 // 3, C3 // 3 // 64, T // W
    fr = _t(rotary_inv_freq() if inv_freq is None else inv_freq, dtype)
    t = _t(qkv, dtype).reshape(B, 3, H, 64, NW, W).permute(1, 0, 2, 4, 5, 3)        # part | B, H, window, step, feature
    q, k, v = t[0], t[1], t[2]
    freqs = torch.einsum("i,j->ij", torch.arange(W).to(dtype), fr)
    freqs = torch.cat([freqs, freqs], dim=-1)                                       # [W, 64]

    def rot(u):
        return torch.cat([-u[..., 32:], u[..., :32]], dim=-1)
    q = q * freqs.cos() + rot(q) * freqs.sin()
    k = k * freqs.cos() + rot(k) * freqs.sin()
    p = torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1)
    o = p @ v                                                                       # B, H, window, step, feature
    return o.permute(0, 1, 4, 2, 3).reshape(B, C, T).contiguous().numpy()


def attn_scores(qkv, W, inv_freq=None):
    """The scaled scores q k^T / 8 of local_attn in binary64 ([B,H,windows,W,W]): the tests state their input ranges with it."""
    B, C3, T = qkv.shape
    H, NW = C3 // 3 // 64, T // W
    fr = _t(rotary_inv_freq() if inv_freq is None else inv_freq)
    t = _t(qkv).reshape(B, 3, H, 64, NW, W).permute(1, 0, 2, 4, 5, 3)
    freqs = torch.einsum("i,j->ij", torch.arange(W).double(), fr)
    freqs = torch.cat([freqs, freqs], dim=-1)
    rot = lambda u: torch.cat([-u[..., 32:], u[..., :32]], dim=-1)
    q = t[0] * freqs.cos() + rot(t[0]) * freqs.sin()
    k = t[1] * freqs.cos() + rot(t[1]) * freqs.sin()
    return (q @ k.transpose(-1, -2) / 8.0).numpy()


def aten_tol(f, M, *args, **kw):
    """Tolerance for an operation without a derived bound (softmax, rsqrt): M times the largest error of ATen's own binary32 CPU answer
    against binary64, computed from the two references alone.  Returns (binary64 answer, tolerance, ATen's largest error)."""
    want = f(*args, dtype=torch.float64, **kw)
    aten = f(*args, dtype=torch.float32, **kw)
    err = float(np.abs(aten.astype(np.float64) - want).max())
    return want, M * err, err


def aten_errors(f, *args, **kw):
    """The two references of aten_tol with the whole error array: (binary64 answer, |ATen's binary32 answer - binary64| per element)."""
    want = f(*args, dtype=torch.float64, **kw)
    return want, np.abs(f(*args, dtype=torch.float32, **kw).astype(np.float64) - want)


# ------------------------------------------------------------------------------------------------------------- quantizers
def vq_distances(z, codebook, kind="dac"):
    """Squared distances of every frame of z [B,D,T] to every row of codebook [N,D] in binary64 -> (dist [B,T,N], argmin [B,T], top-2 gap
    [B,T], bound [B,T,N]).  kind "dac" (DAC / SNAC VectorQuantizer.cs:99-125, as the port computes it: no normalisation) and "euclid"
    (Encodec EuclideanCodebook.cs:155-182, argmax of the negated distance) choose the same index; both are ||z - c||^2 here, written
    directly.  bound: what a binary32 evaluation as (|e|^2 + |c|^2) - 2 e.c may be off by: three D-term chains and two additions."""
    if kind not in ("dac", "euclid"):
        raise ValueError(kind)
    z = np.asarray(z, np.float64); cb = np.asarray(codebook, np.float64)
    B, D, T = z.shape
    e = z.transpose(0, 2, 1).reshape(B * T, D)
    dist = np.empty((B * T, cb.shape[0])); bound = np.empty_like(dist)
    for i in range(0, B * T, 64):                                                    # frame blocks: [64, N, D] temporaries
        diff = e[i:i + 64, None, :] - cb[None, :, :]
        dist[i:i + 64] = (diff * diff).sum(-1)
        ssum = np.abs(e[i:i + 64, None, :]) + np.abs(cb[None, :, :])
        bound[i:i + 64] = dot_bound(D + 2, (ssum * ssum).sum(-1))
    idx = np.argmax(-dist, axis=-1) if kind == "euclid" else np.argmin(dist, axis=-1)
    part = np.partition(dist, 1, axis=-1)
    gap = part[:, 1] - part[:, 0]
    return dist.reshape(B, T, -1), idx.reshape(B, T), gap.reshape(B, T), bound.reshape(B, T, -1)


# ------------------------------------------------------------------------------------------------------------- Encodec (SEANet) layers
# Written from the definitions of the layers (SConv1d / SConvTranspose1d of the EnCodec paper's SEANet with the small-input path as the
# port has it, torch.nn.GroupNorm, torch.nn.LSTM); every function takes `dtype` so that aten_tol can run it in binary32.
def sconv_pad_plan(L, k, stride, causal):
    """SConv1d's padding for rows of L samples -> (left, right, zero_ext).  padding_total = k - stride; extra right padding so that the last
    window is full: n = (L - k + padding_total) / stride + 1, ideal = (ceil(n) - 1) * stride + (k - padding_total), extra = ideal - L;
    causal: all of padding_total on the left, else right = padding_total // 2 and left the rest; `extra` goes to the right.  A row not
    longer than the larger of the two pads cannot be reflected: it is first extended by zeros on the right to max_pad + 1 samples, and that
    extension is NOT trimmed afterwards (deviation D9 of DESIGN.md: the port keeps it, the output is longer)."""
    pt = k - stride
    n = (L - k + pt) / stride + 1
    extra = (int(np.ceil(n)) - 1) * stride + (k - pt) - L
    if causal:
        left, right = pt, extra
    else:
        right = pt // 2
        left, right = pt - right, right + extra
    mx = max(left, right)
    return left, right, (mx - L + 1 if L <= mx else 0)


def sconv_padded(x, k, stride, causal):
    """The padded rows SConv1d convolves: zero extension (small rows), then reflect padding (left, right)."""
    left, right, zext = sconv_pad_plan(x.shape[-1], k, stride, causal)
    if zext:
        x = F.pad(x, (0, zext))
    return F.pad(x, (left, right), mode="reflect") if left or right else x


def two_pass_stats(y, eps=1e-5):
    """(mean, 1 / sqrt(var + eps)) over all but the first axis of y, two passes in binary64 -> [B,2]; also E[x^2] / var per row."""
    y = np.asarray(y, np.float64).reshape(y.shape[0], -1)
    mu = y.mean(axis=1)
    var = ((y - mu[:, None]) ** 2).mean(axis=1)
    with np.errstate(divide="ignore"):
        ratio = (y ** 2).mean(axis=1) / var
    return np.stack([mu, 1.0 / np.sqrt(var + eps)], axis=1), ratio


def _seanet_in(x, x2, elu_in, dtype):
    v = _t(x, dtype)
    if x2 is not None:
        v = v + _t(x2, dtype)
    return F.elu(v) if elu_in else v


def seanet_conv(x, w, b, stride=1, causal=False, gn=None, elu_in=False, x2=None, dtype=torch.float64):
    """[ELU](x [+ x2]) -> SConv1d pad -> conv1d(w [Cout,Cin,K], b) -> [GroupNorm(1, Cout), eps 1e-5, affine gn = (gamma, beta)]."""
    v = sconv_padded(_seanet_in(x, x2, elu_in, dtype), w.shape[2], stride, causal)
    y = F.conv1d(v, _t(w, dtype), _t(b, dtype), stride=stride)
    if gn is not None:
        y = F.group_norm(y, 1, _t(gn[0], dtype), _t(gn[1], dtype), 1e-5)
    return y.numpy()


def seanet_conv_transpose(x, w, b, stride, causal=False, gn=None, elu_in=False, x2=None, dtype=torch.float64):
    """[ELU](x [+ x2]) -> conv_transpose1d(w [Cin,Cout,K], b) -> [GroupNorm(1, Cout) over the UNTRIMMED output] -> trim padding_total =
    K - stride samples: all on the right when causal, else right = padding_total // 2 and the rest on the left."""
    y = F.conv_transpose1d(_seanet_in(x, x2, elu_in, dtype), _t(w, dtype), _t(b, dtype), stride=stride)
    if gn is not None:
        y = F.group_norm(y, 1, _t(gn[0], dtype), _t(gn[1], dtype), 1e-5)
    pt = w.shape[2] - stride
    right = pt if causal else pt // 2
    left = pt - right
    return y[..., left:y.shape[-1] - right].contiguous().numpy()


def slstm_elu(x, layers, dtype=torch.float64):
    """elu(x + LSTM(x)) on x [B,C,T]: torch.nn.LSTM over the time axis, zero initial state; layers = [(w_ih, w_hh, b_ih, b_hh), ...]."""
    C = x.shape[1]
    lstm = torch.nn.LSTM(C, C, num_layers=len(layers)).to(dtype)
    with torch.no_grad():
        for i, (wih, whh, bih, bhh) in enumerate(layers):
            getattr(lstm, f"weight_ih_l{i}").copy_(_t(wih, dtype)); getattr(lstm, f"weight_hh_l{i}").copy_(_t(whh, dtype))
            getattr(lstm, f"bias_ih_l{i}").copy_(_t(bih, dtype)); getattr(lstm, f"bias_hh_l{i}").copy_(_t(bhh, dtype))
        v = _t(x, dtype).permute(2, 0, 1)
        y, _ = lstm(v)
        return F.elu(y + v).permute(1, 2, 0).contiguous().numpy()


def rms_scale(x):
    """Encodec's per-clip scale: sqrt(mean(mono^2)) + 1e-8 with mono the channel mean of x [B,C,T], binary64 -> [B]."""
    mono = np.asarray(x, np.float64).mean(axis=1)
    return np.sqrt((mono ** 2).mean(axis=1)) + 1e-8
