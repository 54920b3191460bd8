"""Incremental DAC / SNAC sessions over the C ABI (nc_session_*, include/nc_mi355x.h "incremental sessions").

    s = dac.decode_session(B, n_quantizers=None)     codes [B, n_q, n] per push            -> pcm [B, 1, n_out]
    s = dac.encode_session(B)                        pcm [B, 1, n] (any n) per push        -> codes [B, n_codebooks, n_out]
    s = snac.decode_session(B)                       list of levels [B, n / stride_i]      -> pcm [B, 1, n_out]
    s = snac.encode_session(B)                       pcm [B, 1, n]                         -> list of levels [B, n_out_i]
    out = s.push(x[, noise]); ...; out = s.flush(); s.reset(); s.pending(); s.close()

The outputs of the pushes and of the flush, concatenated along time, are what the one-shot call on the whole sequence returns, bit for
bit.  Inputs may be numpy arrays (host API, synchronous) or torch CUDA tensors (device API: enqueued on torch's current stream; the
shapes of what comes back follow from frame counts alone, so nothing synchronises).  flush() answers in the form of the last push.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def session_schedule(halo: dict, pushes: Sequence[int], decode: bool = True, flush: bool = True):
    """nc_session_schedule: what a session with these halos (dac_halo / snac_halo) does for pushes of these frame counts -- one dict
    (w0, w1, k0, k1, resident) per push, and one more for the flush.  A host function: no device needed."""
    h = _lib.NcHalo(**{k: int(halo[k]) for k, _ in _lib.NcHalo._fields_})
    p = _lib.i64_array(pushes)
    n = len(p) + (1 if flush else 0)
    steps = (_lib.NcSessionStep * max(1, n))()
    _lib.check(_lib.lib().nc_session_schedule(C.byref(h), 1 if decode else 0, len(p), p, 1 if flush else 0, steps))
    return [{k: int(getattr(steps[i], k)) for k, _ in _lib.NcSessionStep._fields_} for i in range(n)]


class Session:
    """One nc_session on a DAC or SNAC model.  The model must outlive it; calls on one model are serialised by the caller."""

    def __init__(self, model, decode: bool, B: int, n_q: int = 0):
        self._model = model                                # keeps the handle alive
        self.decode, self.B = bool(decode), int(B)
        self._snac = hasattr(model.config, "vq_strides")
        self._s = C.c_void_p()
        _lib.check(_lib.lib().nc_session_create(model._h, 1 if decode else 0, self.B, int(n_q), C.byref(self._s)))
        self._device = None                                # torch device of the last push (None: numpy)

    # ---- lifetime --------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_s", None) is not None and self._s.value:
            try:
                _lib.lib().nc_session_destroy(self._s)
            finally:
                self._s = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self) -> None:
        """After a reset the session is as new: the next push starts another clip."""
        _lib.check(_lib.lib().nc_session_reset(self._s))

    def set_seed(self, seed: int) -> None:
        """Seed of the noise a SNAC decode session draws when push() gets none (per push, from the seed and the frame position: not
        the draw of SNAC.decode(noise=None, seed))."""
        _lib.check(_lib.lib().nc_session_set_seed(self._s, int(seed) & 0xFFFFFFFFFFFFFFFF))

    def pending(self) -> int:
        """Frames pushed and not yet emitted."""
        n = C.c_int64()
        _lib.check(_lib.lib().nc_session_pending(self._s, C.byref(n)))
        return n.value

    def query(self, n_in: int) -> int:
        """Row capacity a push of n_in needs (0: a flush)."""
        n = C.c_int64()
        _lib.check(_lib.lib().nc_session_query(self._s, int(n_in), C.byref(n)))
        return n.value

    # ---- push / flush ----------------------------------------------------------------------
    def _rows(self) -> int:
        return self.B if (self.decode or self._snac) else self.B * self._model.config.n_codebooks

    def _flat(self, parts, dtype: str, what: str):
        """list of [B, ...] arrays / tensors side by side -> one contiguous [B, total] buffer"""
        if any(int(p.shape[0]) != self.B for p in parts):
            raise ValueError(f"{what} must have {self.B} rows")
        if _is_torch(parts[0]):
            import torch
            return torch.cat([p.reshape(self.B, -1).to(getattr(torch, dtype)) for p in parts], dim=1).contiguous()
        return np.ascontiguousarray(np.concatenate([np.asarray(p).reshape(self.B, -1).astype(dtype) for p in parts], axis=1))

    def _shape(self, out, n: int):
        if self.decode:
            return out[:, None, :n]
        if not self._snac:
            return out.reshape(self.B, self._model.config.n_codebooks, -1)[:, :, :n]
        strides = self._model.config.vq_strides
        align = self._align()
        frames = n // sum(align // s for s in strides) * align
        levels, o = [], 0
        for s in strides:
            levels.append(out[:, o:o + frames // s])
            o += frames // s
        return levels

    def _align(self) -> int:
        if not hasattr(self, "_al"):
            from .snac import snac_halo
            self._al = snac_halo(self._model.config)["align"]
        return self._al

    def _run(self, x, n_in: int, nz, flush: bool):
        L = _lib.lib()
        cap = max(1, self.query(0 if flush else n_in))
        n = C.c_int64()
        if self._device is not None:
            import torch
            out = torch.empty((self._rows(), cap), dtype=torch.float32 if self.decode else torch.int64, device=self._device)
            self._model._bind_torch_stream()
            if flush:
                _lib.check(L.nc_session_flush_dev(self._s, out.data_ptr(), cap, C.byref(n)))
            else:
                _lib.check(L.nc_session_push_dev(self._s, x.data_ptr(), n_in, nz.data_ptr() if nz is not None else None, out.data_ptr(), cap, C.byref(n)))
        else:
            out = np.empty((self._rows(), cap), np.float32 if self.decode else np.int64)
            if flush:
                _lib.check(L.nc_session_flush(self._s, out.ctypes.data, cap, C.byref(n)))
            else:
                _lib.check(L.nc_session_push(self._s, x.ctypes.data, n_in, nz.ctypes.data if nz is not None else None, out.ctypes.data, cap, C.byref(n)))
        return self._shape(out, n.value)

    def push(self, x, noise: Optional[Sequence] = None):
        """The next codes (decode) or PCM (encode); returns what became final, which may be empty.  noise (SNAC decode sessions of a
        model with NoiseBlocks): the blocks for the pushed frames, SNAC.noise_shapes(B, n)."""
        if x is None:
            raise ValueError("the pushed data must not be null")
        if self.decode:
            if self._snac:
                if len(x) != len(self._model.config.vq_strides):
                    raise ValueError(f"Expected {len(self._model.config.vq_strides)} codebooks but got {len(x)}")
                n_in = int(x[-1].shape[-1]) * self._model.config.vq_strides[-1]
                if [int(np.prod(c.shape[1:])) * s for c, s in zip(x, self._model.config.vq_strides)] != [n_in] * len(x):
                    raise ValueError("code level widths do not match one frame count")
                first = x[0]
                flat = self._flat(list(x), "int64", "codes")
            else:
                if x.ndim != 3 or int(x.shape[0]) != self.B:
                    raise ValueError(f"codes must be [{self.B},n_q,n]")
                n_in, first = int(x.shape[2]), x
                flat = self._flat([x], "int64", "codes")
        else:
            if x.ndim not in (2, 3) or int(x.shape[0]) != self.B or (x.ndim == 3 and x.shape[1] != 1):
                raise ValueError(f"audio must be [{self.B},1,n]")
            n_in, first = int(x.shape[-1]), x
            flat = self._flat([x], "float32", "audio")
        self._device = first.device if _is_torch(first) else None
        nz = None
        if noise is not None and self.decode and self._snac and self._model.config.noise:
            shapes = self._model.noise_shapes(self.B, n_in)
            if [int(np.prod(a.shape)) for a in noise] != [int(np.prod(sh)) for sh in shapes]:
                raise ValueError(f"noise shapes must be {shapes}")
            if self._device is not None:
                import torch
                nz = torch.cat([torch.as_tensor(a, dtype=torch.float32).reshape(-1).to(self._device) for a in noise]).contiguous()
            else:
                nz = np.ascontiguousarray(np.concatenate([np.asarray(a, np.float32).reshape(-1) for a in noise]))
        return self._run(flat, n_in, nz, False)

    def flush(self):
        """The end of the clip: returns everything not yet emitted.  Afterwards only reset() or close()."""
        return self._run(None, 0, None, True)
