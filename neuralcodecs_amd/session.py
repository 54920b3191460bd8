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


class _Flush:
    def __repr__(self):
        return "FLUSH"


FLUSH = _Flush()    # the value of a slot in SessionPool.step that ends the slot's clip


def session_pool_plan(halo: dict, pushed: Sequence[int], emitted: Sequence[int], push_frames: Sequence[int], decode: bool = True, max_rows: int = 0):
    """nc_session_pool_plan: how a pool step groups streams that have pushed[i] / emitted[i] frames and push push_frames[i] more (0: the
    flush) -- (steps, group_of, n_groups): one dict per stream as session_schedule gives them, the batch each window runs in (-1: no
    window).  A host function: no device needed."""
    h = _lib.NcHalo(**{k: int(halo[k]) for k, _ in _lib.NcHalo._fields_})
    n = len(pushed)
    if not (len(emitted) == len(push_frames) == n):
        raise ValueError("pushed, emitted and push_frames must have one entry per stream")
    steps = (_lib.NcSessionStep * max(1, n))()
    group_of = (C.c_int32 * max(1, n))()
    n_groups = C.c_int32()
    _lib.check(_lib.lib().nc_session_pool_plan(C.byref(h), 1 if decode else 0, n, _lib.i64_array(pushed), _lib.i64_array(emitted),
                                               _lib.i64_array(push_frames), int(max_rows), steps, group_of, C.byref(n_groups)))
    return ([{k: int(getattr(steps[i], k)) for k, _ in _lib.NcSessionStep._fields_} for i in range(n)], [int(group_of[i]) for i in range(n)],
            n_groups.value)


class SessionPool:
    """One nc_session_pool on a DAC or SNAC model: n_slots independent streams, one direction.  step() advances any subset of slots, each
    by its own amount; what a slot returns is what a B = 1 Session returns for the same pushes, bit for bit.

        pool = dac.decode_pool(n_slots, n_q=None) | dac.encode_pool(n_slots) | snac.decode_pool(n_slots) | snac.encode_pool(n_slots)
        out = pool.step({slot: x | FLUSH, ...}[, noise={slot: blocks}])      x as Session.push takes it for B = 1
        pool.reset(slot); pool.set_seed(slot, seed); pool.pending(slot); pool.query({slot: n_in | 0}); pool.close()

    Inputs are numpy arrays (host API, synchronous) or torch CUDA tensors (device API on torch's current stream: output shapes follow
    from frame counts alone, so nothing synchronises).  A step of flushes alone answers in the form of the last step with data."""

    def __init__(self, model, decode: bool, n_slots: int, n_q: int = 0):
        self._model = model                                # keeps the handle alive
        self.decode, self.n_slots = bool(decode), int(n_slots)
        self._snac = hasattr(model.config, "vq_strides")
        self._nq = int(n_q) if (decode and not self._snac) else 0
        self._p = C.c_void_p()
        _lib.check(_lib.lib().nc_session_pool_create(model._h, 1 if decode else 0, self.n_slots, int(n_q), C.byref(self._p)))
        self._device = None

    # ---- lifetime --------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_p", None) is not None and self._p.value:
            try:
                _lib.lib().nc_session_pool_destroy(self._p)
            finally:
                self._p = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, slot: int) -> None:
        """After a reset the slot is as new: its next push starts another clip."""
        _lib.check(_lib.lib().nc_session_pool_reset_slot(self._p, int(slot)))

    def set_seed(self, slot: int, seed: int) -> None:
        """Seed of the noise the slot of a SNAC decode pool draws when step() gets none: slot seed s equals a B = 1 Session with seed s."""
        _lib.check(_lib.lib().nc_session_pool_set_seed(self._p, int(slot), int(seed) & 0xFFFFFFFFFFFFFFFF))

    def pending(self, slot: int) -> int:
        """Frames the slot has pushed and not yet emitted."""
        n = C.c_int64()
        _lib.check(_lib.lib().nc_session_pool_pending(self._p, int(slot), C.byref(n)))
        return n.value

    def query(self, n_in: dict) -> dict:
        """{slot: n_in (0: flush)} -> {slot: the exact n_out per row a step of these entries would return now}"""
        slots = (C.c_int32 * max(1, len(n_in)))(*[int(s) for s in n_in])
        nin = _lib.i64_array(n_in.values())
        out = (C.c_int64 * max(1, len(n_in)))()
        _lib.check(_lib.lib().nc_session_pool_query(self._p, len(n_in), slots, nin, out))
        return {int(s): int(out[i]) for i, s in enumerate(n_in)}

    # ---- step ------------------------------------------------------------------------------
    def _out_rows(self) -> int:
        return 1 if (self.decode or self._snac) else self._model.config.n_codebooks

    def _entry(self, x):
        """(n_in, flat parts, first array) of one slot's data"""
        cfg = self._model.config
        if self.decode and self._snac:
            if len(x) != len(cfg.vq_strides):
                raise ValueError(f"Expected {len(cfg.vq_strides)} codebooks but got {len(x)}")
            n_in = int(np.prod(x[-1].shape)) * cfg.vq_strides[-1]
            if [int(np.prod(c.shape)) * s for c, s in zip(x, cfg.vq_strides)] != [n_in] * len(x):
                raise ValueError("code level widths do not match one frame count")
            return n_in, list(x), x[0]
        if self.decode:
            nq = self._nq or cfg.n_codebooks
            if x.ndim not in (2, 3) or (x.ndim == 3 and int(x.shape[0]) != 1) or int(x.shape[-2]) != nq:
                raise ValueError(f"codes of a slot must be [1,{nq},n]")
            return int(x.shape[-1]), [x], x
        if x.ndim not in (1, 2, 3) or any(int(d) != 1 for d in x.shape[:-1]):
            raise ValueError("audio of a slot must be [1,1,n]")
        return int(x.shape[-1]), [x], x

    def _shape(self, flat, n: int):
        if self.decode:
            return flat.reshape(1, 1, n)
        if not self._snac:
            return flat.reshape(1, self._model.config.n_codebooks, n)
        strides = self._model.config.vq_strides
        if not hasattr(self, "_al"):
            from .snac import snac_halo
            self._al = snac_halo(self._model.config)["align"]
        frames = n // sum(self._al // s for s in strides) * self._al
        levels, o = [], 0
        for s in strides:
            levels.append(flat[o:o + frames // s].reshape(1, -1))
            o += frames // s
        return levels

    def step(self, entries: dict, noise: Optional[dict] = None) -> dict:
        """{slot: the next codes (decode) or PCM (encode) | FLUSH} -> {slot: what became final for that slot (may be empty)}.  noise (SNAC
        decode pools of a model with NoiseBlocks): {slot: blocks for the pushed frames, SNAC.noise_shapes(1, n)} for every pushing slot,
        or None: every slot draws its own from its seed and frame position."""
        if not entries:
            raise ValueError("a step needs at least one slot")
        L = _lib.lib()
        slots, n_in, parts, nz_parts, first = [], [], [], [], None
        with_noise = noise is not None and self.decode and self._snac and bool(self._model.config.noise)
        for slot, x in entries.items():
            slots.append(int(slot))
            if x is FLUSH:
                n_in.append(0)
                continue
            if x is None:
                raise ValueError("the pushed data must not be null (FLUSH ends a clip)")
            n, ps, f = self._entry(x)
            if n <= 0:
                raise ValueError("a push must not be empty")
            first = f if first is None else first
            n_in.append(n)
            parts += ps
            if with_noise:
                shapes = self._model.noise_shapes(1, n)
                blocks = noise.get(slot)
                if blocks is None or [int(np.prod(a.shape)) for a in blocks] != [int(np.prod(sh)) for sh in shapes]:
                    raise ValueError(f"noise of slot {slot} must have the shapes {shapes}")
                nz_parts += list(blocks)
        if first is not None:
            self._device = first.device if _is_torch(first) else None
        c_slots = (C.c_int32 * len(slots))(*slots)
        c_nin = _lib.i64_array(n_in)
        n_out = (C.c_int64 * len(slots))()
        _lib.check(L.nc_session_pool_query(self._p, len(slots), c_slots, c_nin, n_out))
        rows = self._out_rows()
        sizes = [rows * int(v) for v in n_out]
        cap = max(1, sum(sizes))
        in_dt, out_dt = ("int64", "float32") if self.decode else ("float32", "int64")
        if self._device is not None:
            import torch
            flat = torch.cat([p.reshape(-1).to(getattr(torch, in_dt)) for p in parts]).contiguous() if parts else None
            nz = torch.cat([torch.as_tensor(a, dtype=torch.float32).reshape(-1).to(self._device) for a in nz_parts]).contiguous() if nz_parts else None
            out = torch.empty((cap,), dtype=getattr(torch, out_dt), device=self._device)
            self._model._bind_torch_stream()
            _lib.check(L.nc_session_pool_step_dev(self._p, len(slots), c_slots, c_nin, flat.data_ptr() if flat is not None else None,
                                                  nz.data_ptr() if nz is not None else None, out.data_ptr(), cap, n_out))
        else:
            flat = np.ascontiguousarray(np.concatenate([np.asarray(p).reshape(-1).astype(in_dt) for p in parts])) if parts else None
            nz = np.ascontiguousarray(np.concatenate([np.asarray(a, np.float32).reshape(-1) for a in nz_parts])) if nz_parts else None
            out = np.empty((cap,), out_dt)
            _lib.check(L.nc_session_pool_step(self._p, len(slots), c_slots, c_nin, flat.ctypes.data if flat is not None else None,
                                              nz.ctypes.data if nz is not None else None, out.ctypes.data, cap, n_out))
        res, o = {}, 0
        for slot, v, sz in zip(slots, n_out, sizes):
            res[slot] = self._shape(out[o:o + sz], int(v))
            o += sz
        return res
