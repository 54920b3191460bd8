"""Op-level test hooks over the engine's kernels (nc_op_* in include/nc_mi355x.h): host numpy in/out."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


def _p(a):
    return None if a is None else a.ctypes.data


def conv1d(x, weight, bias=None, stride=1, pad=0, dil=1, alpha_in=None, alpha_out=None, residual=None, transposed=False,
           out_pad=0, tanh_out=False, device_index=0):
    x = np.ascontiguousarray(x, np.float32); w = np.ascontiguousarray(weight, np.float32)
    B, Cin, Tin = x.shape
    if transposed:
        Cout, K = w.shape[1], w.shape[2]
        Tout = (Tin - 1) * stride - 2 * pad + K + out_pad
    else:
        Cout, K = w.shape[0], w.shape[2]
        Tout = (Tin + 2 * pad - dil * (K - 1) - 1) // stride + 1
    d = _lib.NcConvDesc(B, Cin, Cout, K, stride, pad, dil, out_pad, Tin, 1 if transposed else 0, 1 if tanh_out else 0)
    f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    b, ai, ao, r = f(bias), f(alpha_in), f(alpha_out), f(residual)
    y = np.empty((B, Cout, Tout), np.float32)
    to = C.c_int64()
    _lib.check(_lib.lib().nc_op_conv1d(device_index, C.byref(d), x.ctypes.data, w.ctypes.data, _p(b), _p(ai), _p(ao), _p(r),
                                       y.ctypes.data, C.byref(to)))
    assert to.value == Tout
    return y


def res_unit(x, w7, b7, a1, a2, w1, b1, dil=1, fused=True, iters=0, device_index=0):
    """One DAC ResidualUnit; returns y (and the average ms per repetition when iters > 0)."""
    f = lambda a: np.ascontiguousarray(a, np.float32)
    x, w7, b7, a1, a2, w1, b1 = map(f, (x, w7, b7, a1, a2, w1, b1))
    B, Cc, T = x.shape
    y = np.empty_like(x)
    ms = C.c_double()
    _lib.check(_lib.lib().nc_op_res_unit(device_index, B, Cc, T, dil, x.ctypes.data, w7.ctypes.data, b7.ctypes.data, a1.ctypes.data,
                                         a2.ctypes.data, w1.ctypes.data, b1.ctypes.data, 1 if fused else 0, y.ctypes.data, iters,
                                         C.byref(ms)))
    return (y, ms.value) if iters > 0 else y


def vq_argmin(z_e, codebook, device_index=0):
    z = np.ascontiguousarray(z_e, np.float32); cb = np.ascontiguousarray(codebook, np.float32)
    B, D, T = z.shape
    idx = np.empty((B, T), np.int64); st = np.empty_like(z)
    _lib.check(_lib.lib().nc_op_vq_argmin(device_index, z.ctypes.data, B, D, T, cb.ctypes.data, cb.shape[0], idx.ctypes.data,
                                          st.ctypes.data))
    return idx, st


def euclid_rvq(residual, codebooks, form=1, device_index=0):
    """Encodec RVQ encode on residual [B,D,T] with codebooks [n_q,N,D] -> (codes [B,n_q,T], residual after the last stage)."""
    r = np.ascontiguousarray(residual, np.float32); cb = np.ascontiguousarray(codebooks, np.float32)
    B, D, T = r.shape
    nq, N, _ = cb.shape
    codes = np.empty((B, nq, T), np.int64); out = np.empty_like(r)
    _lib.check(_lib.lib().nc_op_euclid_rvq(device_index, r.ctypes.data, B, D, T, cb.ctypes.data, nq, N, int(form), codes.ctypes.data, out.ctypes.data))
    return codes, out


def dac_rvq(residual, w_in, b_in, codebooks, w_out, b_out, form=1, out=None, device_index=0):
    """The DAC quantizer on residual [B,L,T] with folded weights w_in [n_q,D,L], b_in [n_q,D], codebooks [n_q,N,D], w_out [n_q,L,D],
    b_out [n_q,L] -> (codes [B,n_q,T], zq [B,L,T], latents [B,n_q*D,T]).  form=1: all stages in one launch (NcError status
    NC_EUNSUPPORTED where that kernel has no instance); form=0: the launches per stage.  out=(codes, zq, latents): arrays to fill; the
    call then returns the raw status instead of raising (the refusal tests look at what an error leaves in them)."""
    r = _f(residual); wi = _f(w_in); cb = _f(codebooks); wo = _f(w_out); bi = _f(b_in); bo = _f(b_out)
    B, L, T = r.shape
    nq, N, D = cb.shape
    if nq and out is None:
        assert wi.shape == (nq, D, L) and wo.shape == (nq, L, D) and (bi is None or bi.shape == (nq, D)) and (bo is None or bo.shape == (nq, L))
    if out is None:
        codes = np.empty((B, nq, T), np.int64); zq = np.empty_like(r); lat = np.empty((B, nq * D, T), np.float32)
    else:
        codes, zq, lat = out
    st = _lib.lib().nc_op_dac_rvq(device_index, r.ctypes.data, B, L, T, nq, N, D, wi.ctypes.data, _p(bi), cb.ctypes.data, wo.ctypes.data, _p(bo),
                                  int(form), codes.ctypes.data, zq.ctypes.data, lat.ctypes.data)
    if out is not None:
        return st
    _lib.check(st)
    return codes, zq, lat


def rvq_update(q, zq, residual=None, s=1, first=False, device_index=0):
    """SNAC's quantizer update on q [rows,T/s], zq [rows,T], residual [rows,T] or None: returns (zq', residual' or None) with
    zq' = (0 if first else zq) + repeat(q, s) and residual' = residual - repeat(q, s); the inputs are left as they are."""
    q = _f(q); zq = _f(zq).copy(); r = None if residual is None else _f(residual).copy()
    rows, T = zq.shape
    assert q.shape == (rows, T // s) and (r is None or r.shape == zq.shape)
    _lib.check(_lib.lib().nc_op_rvq_update(device_index, q.ctypes.data, zq.ctypes.data, _p(r), rows, T, int(s), 1 if first else 0))
    return zq, r


def vq_gather(codebook, codes_flat, codes_offset, codes_bstride, B, T, guard=0, fill=0.0, device_index=0):
    """out[b,d,t] = codebook[codes_flat[codes_offset + b * codes_bstride + t]][d] (a code outside [0, N) is clamped) -> the whole output
    buffer, flat: `guard` floats of `fill`, out [B,D,T], `guard` floats of `fill`, all of it through the device and back."""
    cb = _f(codebook); codes = np.ascontiguousarray(codes_flat, np.int64).reshape(-1)
    N, D = cb.shape
    assert codes_offset >= 0 and codes_bstride >= T and codes_offset + (B - 1) * codes_bstride + T <= codes.size
    buf = np.full(B * D * T + 2 * guard, fill, np.float32)
    _lib.check(_lib.lib().nc_op_vq_gather(device_index, cb.ctypes.data, N, D, codes.ctypes.data, int(codes_offset), int(codes_bstride), B, T,
                                          buf.ctypes.data + 4 * guard, int(guard)))
    return buf


def encodec_trace_taps(model):
    """Number of taps of either stack of a loaded Encodec model (3 + 4 * len(ratios))."""
    n = C.c_int32()
    _lib.check(_lib.lib().nc_op_encodec_trace(model._h, 0, None, 0, 0, -1, None, None, None, None, C.byref(n), None))
    return n.value


def encodec_trace(model, x, tap, decoder=False):
    """Tap `tap` of the SEANet encoder on x [B,channels,L] (no RMS normalisation) or, decoder=True, of the decoder on x [B,dimension,L], by
    the launches the model itself makes: (tap [B,C,L'] with its pending GroupNorm applied and no ELU, stats [B,2] = (mean, rstd) of that
    GroupNorm or None).  Tap order: see nc_op_encodec_trace in include/nc_mi355x.h."""
    x = np.ascontiguousarray(x, np.float32)
    B, _, L = x.shape
    Co, Lo, hs = C.c_int32(), C.c_int64(), C.c_int32()
    f = _lib.lib().nc_op_encodec_trace
    _lib.check(f(model._h, int(bool(decoder)), None, B, L, int(tap), None, None, C.byref(Co), C.byref(Lo), None, None))
    out = np.empty((B, Co.value, Lo.value), np.float32); st = np.empty((B, 2), np.float32)
    _lib.check(f(model._h, int(bool(decoder)), x.ctypes.data, B, L, int(tap), out.ctypes.data, st.ctypes.data, None, None, None, C.byref(hs)))
    return out, (st if hs.value else None)


def encodec_lstm_carried(model, x, state=None, decoder=False):
    """nc_op_encodec_lstm_carried: one SLSTM stack of a loaded Encodec model on x [N,C,T] from `state` = (h, c), each [N,layers,C]
    (None: the zero state) -> (y [N,C,T] = elu?(x + lstm(x)) as the LSTM tap, (h, c) behind the last step)."""
    x = np.ascontiguousarray(x, np.float32)
    N, Cc, T = x.shape
    nl = model.config.lstm_layers
    if state is None:
        h, c = np.zeros((N, nl, Cc), np.float32), np.zeros((N, nl, Cc), np.float32)
    else:
        h, c = (np.array(s, dtype=np.float32, order="C", copy=True).reshape(N, nl, Cc) for s in state)
    y = np.empty_like(x)
    _lib.check(_lib.lib().nc_op_encodec_lstm_carried(model._h, int(bool(decoder)), x.ctypes.data, N, T, h.ctypes.data, c.ctypes.data, y.ctypes.data))
    return y, (h, c)


def concat_copy(a, b, dst, desc, device_index=0):
    """nc_op_concat_copy: for every row (a_off, na, b_off, nb, s0, dst_off, n) of desc, dst[dst_off : dst_off + n] =
    (a[a_off : a_off + na] ++ b[b_off : b_off + nb] ++ zeros)[s0 : s0 + n], all rows in one launch.  a, b, dst: 1-D float32 or int64 of
    one dtype; returns a copy of dst with the rows written."""
    out = np.array(dst, order="C", copy=True)
    a = np.ascontiguousarray(a, out.dtype); b = np.ascontiguousarray(b, out.dtype)
    desc = np.ascontiguousarray(desc, np.int64).reshape(-1, 7)
    _lib.check(_lib.lib().nc_op_concat_copy(device_index, out.dtype.itemsize, a.ctypes.data, a.size, b.ctypes.data, b.size, out.ctypes.data, out.size,
                                            desc.ctypes.data, desc.shape[0]))
    return out


def fold_weight_norm(v, g):
    v = np.ascontiguousarray(v, np.float32); g = np.ascontiguousarray(g, np.float32).reshape(-1)
    w = np.empty_like(v)
    _lib.check(_lib.lib().nc_op_fold_weight_norm(v.ctypes.data, g.ctypes.data, v.shape[0], int(np.prod(v.shape[1:])), w.ctypes.data))
    return w


def _f(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def dwconv1d(x, weight, bias=None, pad=0, dil=1, alpha_in=None, alpha_out=None, device_index=0):
    """Depthwise convolution on x [B,C,T] with weight [C,K] (or [C,1,K]): the first T outputs over the zero-extended rows."""
    x = _f(x); w = _f(weight).reshape(x.shape[1], -1)
    B, Cc, T = x.shape
    b, ai, ao = _f(bias), _f(alpha_in), _f(alpha_out)
    y = np.empty_like(x)
    _lib.check(_lib.lib().nc_op_dwconv1d(device_index, B, Cc, T, w.shape[1], pad, dil, x.ctypes.data, w.ctypes.data, _p(b), _p(ai), _p(ao),
                                         y.ctypes.data))
    return y


def layer_norm(x, gamma, beta, device_index=0):
    """LayerNorm over the channel axis of x [B,C,T] (eps 1e-5)."""
    x, g, b = _f(x), _f(gamma), _f(beta)
    B, Cc, T = x.shape
    assert g.size == Cc and b.size == Cc
    y = np.empty_like(x)
    _lib.check(_lib.lib().nc_op_layer_norm(device_index, B, Cc, T, x.ctypes.data, g.ctypes.data, b.ctypes.data, y.ctypes.data))
    return y


def local_attn(qkv, window, inv_freq, device_index=0):
    """Windowed rotary attention on qkv [B,3C,T] -> [B,C,T]; inv_freq [32] is the checkpoint's rel_pos.inv_freq buffer."""
    qkv = _f(qkv); fr = _f(inv_freq)
    B, C3, T = qkv.shape
    assert C3 % 3 == 0 and fr.size == 32
    y = np.empty((B, C3 // 3, T), np.float32)
    _lib.check(_lib.lib().nc_op_local_attn(device_index, B, C3 // 3, T, int(window), qkv.ctypes.data, _p(fr), y.ctypes.data))
    return y


def avg_pool(x, s, device_index=0):
    """avg_pool1d(s) on x [rows,T] -> [rows,T // s]."""
    x = _f(x)
    rows, T = x.shape
    y = np.empty((rows, T // s), np.float32)
    _lib.check(_lib.lib().nc_op_avg_pool(device_index, rows, T, int(s), x.ctypes.data, y.ctypes.data))
    return y


def snac_unit(x, w7, b7, a1, a2, w1, b1=None, alpha_next=None, dil=1, fused=True, device_index=0):
    """One depthwise SNAC ResidualUnit on x [B,C,T]: w7 [C,7] (or [C,1,7]), w1 [C,C] (or [C,C,1]); fused=True is the one-launch kernel
    (NcError status NC_EUNSUPPORTED where it does not serve the shape), fused=False the two-launch path."""
    x = _f(x)
    B, Cc, T = x.shape
    w7 = _f(w7).reshape(Cc, 7); w1 = _f(w1).reshape(Cc, Cc)
    b7, a1, a2, b1, an = _f(b7), _f(a1), _f(a2), _f(b1), _f(alpha_next)
    y = np.empty_like(x)
    _lib.check(_lib.lib().nc_op_snac_unit(device_index, B, Cc, T, dil, x.ctypes.data, w7.ctypes.data, _p(b7), a1.ctypes.data, a2.ctypes.data,
                                          w1.ctypes.data, _p(b1), _p(an), 1 if fused else 0, y.ctypes.data))
    return y
