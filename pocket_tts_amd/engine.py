"""Python host wrapper over the C ABI (include/ptts.h).  PyTorch-ROCm is used only for device
memory and streams; all arithmetic of the hot path runs in libptts.so.

Mirrors the reference's internal seam:
  * `Engine.lm_prefill / lm_decode_step`  <->  `TTSModel._run_flow_lm_and_increment_step`
    (reference tts_model.py:317-346)
  * `Engine.mimi_decode`                  <->  the body of `_decode_audio_worker`
    (reference tts_model.py:444-455) = de-normalise + quantizer + `MimiModel.decode_from_latent`
  * `LMState` / `MimiState`               <->  `init_states(...)` dicts (reference stateful_module.py:7-16)
"""

from __future__ import annotations

import ctypes as C
import numbers
import os
import weakref

import numpy as np
import torch

from . import _lib
from .config import Config
from .weights import mimi_encode_spec, state_dict_spec


def _ptr(t: torch.Tensor | None):
    return None if t is None else C.c_void_p(t.data_ptr())


def make_ptts_config(cfg: Config) -> _lib.PttsConfig:
    t, m, sn = cfg.flow_lm.transformer, cfg.mimi.transformer, cfg.mimi.seanet
    if len(sn.ratios) != 3:
        raise ValueError("SEANet decoder with 3 upsampling stages expected")
    pc = _lib.PttsConfig()
    pc.d_model, pc.num_heads, pc.num_layers = t.d_model, t.num_heads, t.num_layers
    pc.ff_dim = t.d_model * t.hidden_scale
    pc.ldim = cfg.mimi.quantizer.dimension
    pc.flow_dim, pc.flow_depth = cfg.flow_lm.flow.dim, cfg.flow_lm.flow.depth
    pc.max_period = float(t.max_period)
    pc.m_dim, pc.m_heads, pc.m_layers, pc.m_ff = m.d_model, m.num_heads, m.num_layers, m.dim_feedforward
    pc.m_context = m.context
    pc.m_max_period = float(m.max_period)
    pc.n_filters = sn.n_filters
    pc.ratios = (C.c_int32 * 3)(*[int(r) for r in sn.ratios])
    pc.kernel_size, pc.res_kernel_size, pc.last_kernel_size = sn.kernel_size, sn.residual_kernel_size, sn.last_kernel_size
    pc.compress = sn.compress
    pc.upsample_stride = cfg.upsample_stride
    return pc


_MASK64 = (1 << 64) - 1


def _mix64(z: int) -> int:
    """the splitmix64 finaliser the device generator hashes with (mix64 in csrc/ptts_kernels.h)"""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def check_seed(seed, bits: int = 63) -> int:
    """`seed` as an int in [0, 2**bits), else ValueError (bool, float, negative and too large values are refused)"""
    if isinstance(seed, bool) or not isinstance(seed, numbers.Integral) or not 0 <= int(seed) < (1 << bits):
        raise ValueError(f"seed must be an integer in [0, 2**{bits}), got {seed!r}")
    return int(seed)


def chunk_seed(seed: int, chunk: int) -> int:
    """The 64-bit row seed (`LMState.set_row_seed`) of text chunk `chunk` of a request seeded `seed` (an int in
    [0, 2**63)); every entry point derives its row seeds here.  Chunk 0 uses the request's seed itself.  Later chunks hash
    seed and index: the generator hashes `seed + C * key` with C = 0x9E3779B97F4A7C15, so seeds an additive step apart
    could yield shifted copies of one stream."""
    seed = check_seed(seed)
    if isinstance(chunk, bool) or not isinstance(chunk, numbers.Integral) or not 0 <= int(chunk) < (1 << 32):
        raise ValueError(f"chunk index must be an integer in [0, 2**32), got {chunk!r}")
    if chunk == 0:
        return seed
    return _mix64(_mix64(seed) ^ int(chunk))


def pad_token_rows(rows, pad_id: int = 0):
    """Token rows of different lengths -> (ids int64 [n, t_max], lengths): row i holds `rows[i]` (a tensor or sequence of
    ids, [T] or [1, T]) followed by `pad_id`, which must be a valid id (`Engine.embed_text` refuses ids outside the
    table); the padding's embeddings are what `Engine.lm_prefill(..., lengths=)` ignores."""
    flat = [torch.as_tensor(r, dtype=torch.int64).reshape(-1) for r in rows]
    if not flat:
        raise ValueError("need at least one token row")
    lengths = [int(r.numel()) for r in flat]
    ids = torch.full((len(flat), max(max(lengths), 1)), int(pad_id), dtype=torch.int64)
    for i, r in enumerate(flat):
        ids[i, :lengths[i]] = r
    return ids, lengths


class LMState:
    """FlowLM KV caches of `batch` sequences with capacity `t_cap` positions."""

    def __init__(self, engine: "Engine", batch: int, t_cap: int):
        self.engine, self.batch, self.t_cap = engine, batch, t_cap
        h = C.c_void_p()
        _lib.check(engine.lib.ptts_lm_state_create(engine.handle, batch, t_cap, C.byref(h)))
        self.handle = h
        engine._states.add(self)

    def close(self):
        if self.handle is not None:
            self.engine.lib.ptts_lm_state_destroy(self.handle)
            self.handle = None

    def reset(self):
        _lib.check(self.engine.lib.ptts_lm_state_reset(self.handle, self.engine._sp))

    def set_noise(self, temp: float, seed: int = 0):
        """device-side N(0, temp) noise for steps called with noise=None (perf runs)"""
        _lib.check(self.engine.lib.ptts_lm_set_noise(self.handle, float(temp), int(seed)))

    def set_row_sampling(self, row: int, temp: float, noise_clamp: float | None = None, eos_threshold: float = -4.0):
        """Row `row` draws with its own temperature (and, with `noise_clamp` > 0, a truncated normal) and compares its EOS
        logit with its own threshold; read by the kernels at run time, so captured steps pick it up (include/ptts.h)."""
        clamp = 0.0 if noise_clamp is None else float(noise_clamp)
        _lib.check(self.engine.lib.ptts_lm_state_set_row_sampling(self.handle, row, float(temp), clamp,
                                                                  float(eos_threshold), self.engine._sp))

    def clear_row_sampling(self, row: int):
        """row `row` returns to the state's temperature (`set_noise`) and the step's EOS threshold"""
        _lib.check(self.engine.lib.ptts_lm_state_clear_row_sampling(self.handle, row, self.engine._sp))

    def set_row_seed(self, row: int, seed: int):
        """Row `row` draws from its own stream: its j-th step from now on is keyed by (seed, j, column), whatever the row
        index, the batch and the state's own seed and step counter (include/ptts.h).  Restarts the row's stream; read by
        the kernels at run time, so captured steps pick it up."""
        _lib.check(self.engine.lib.ptts_lm_state_set_row_seed(self.handle, row, check_seed(seed, bits=64),
                                                              self.engine._sp))

    def clear_row_seed(self, row: int):
        """row `row` returns to the state's seed and step counter (`set_noise`)"""
        _lib.check(self.engine.lib.ptts_lm_state_clear_row_seed(self.handle, row, self.engine._sp))

    def reserve_row_lsd(self, K: int):
        """Per-row LSD schedules of up to `K` Euler steps (include/ptts.h); before any graph of this state is captured"""
        _lib.check(self.engine.lib.ptts_lm_state_reserve_row_lsd(self.handle, int(K), self.engine._sp))

    def set_row_lsd(self, row: int, n: int):
        """row `row` runs `n` (1 <= n <= the reserved K) Euler steps of the flow head instead of the step's lsd_steps;
        read by the kernels at run time, so captured steps pick it up"""
        _lib.check(self.engine.lib.ptts_lm_state_set_row_lsd(self.handle, row, int(n), self.engine._sp))

    def clear_row_lsd(self, row: int):
        """row `row` returns to the step's lsd_steps"""
        _lib.check(self.engine.lib.ptts_lm_state_clear_row_lsd(self.handle, row, self.engine._sp))

    def set_flow_fold(self, on: bool):
        """Flow fold (include/ptts.h): the flow cluster computes the AdaLN modulations inside its hand-off waits and the
        `flow.adaln` launch goes, where the state qualifies; before any graph of this state is captured"""
        _lib.check(self.engine.lib.ptts_lm_state_set_flow_fold(self.handle, int(bool(on)), self.engine._sp))

    def error(self) -> bool:
        """True after a cooperative kernel of this state gave up waiting for a peer workgroup"""
        r = self.engine.lib.ptts_lm_state_error(self.handle, self.engine._sp)
        _lib.check(min(int(r), 0))
        return bool(r)

    def offsets(self) -> np.ndarray:
        out = (C.c_int32 * self.batch)()
        _lib.check(self.engine.lib.ptts_lm_state_offsets(self.handle, out, self.engine._sp))
        return np.array(out[:], dtype=np.int64)

    def import_layer(self, layer: int, cache: torch.Tensor, t: int):
        """cache: f32[2, Bsrc, >=t, H, 64] in the reference layout (reference transformer.py:32-36)."""
        e = self.engine
        if cache.dim() != 5 or cache.shape[0] != 2 or cache.shape[1] not in (1, self.batch) or cache.shape[2] < t \
                or cache.shape[3] != e.H or cache.shape[4] != 64:
            raise ValueError(f"voice-state cache of layer {layer}: expected [2, 1|{self.batch}, >={t}, {e.H}, 64], "
                             f"got {tuple(cache.shape)}")
        cache = cache[:, :, :t].to(self.engine.device, torch.float32).contiguous()
        self.engine._pre()
        _lib.check(self.engine.lib.ptts_lm_state_import(self.handle, layer, _ptr(cache), cache.shape[1], t, self.engine._sp))
        self.engine.sync()

    def export_layer(self, layer: int, t: int) -> torch.Tensor:
        e = self.engine
        out = torch.empty((2, self.batch, t, e.H, 64), dtype=torch.float32, device=e.device)
        _lib.check(e.lib.ptts_lm_state_export(self.handle, layer, _ptr(out), t, e._sp))
        e.sync()
        return out

    def copy_row_from(self, row: int, src: "LMState", src_row: int = 0):
        """row `row` <- sequence `src_row` of `src`; rows may have different lengths"""
        _lib.check(self.engine.lib.ptts_lm_state_copy_row_from(self.handle, row, src.handle, src_row, self.engine._sp))

    def copy_from(self, src: "LMState"):
        _lib.check(self.engine.lib.ptts_lm_state_copy(self.handle, src.handle, self.engine._sp))

    def set_row_active(self, row: int, active: bool):
        """continuous batching: a parked row stays at position 0 (copy_row_from re-activates it)"""
        _lib.check(self.engine.lib.ptts_lm_state_set_row_active(self.handle, row, int(bool(active)), self.engine._sp))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MimiState:
    def __init__(self, engine: "Engine", batch: int):
        self.engine, self.batch = engine, batch
        h = C.c_void_p()
        _lib.check(engine.lib.ptts_mimi_state_create(engine.handle, batch, C.byref(h)))
        self.handle = h
        engine._states.add(self)

    def close(self):
        if self.handle is not None:
            self.engine.lib.ptts_mimi_state_destroy(self.handle)
            self.handle = None

    def reset(self, stream: torch.cuda.Stream | None = None):
        sp = self.engine._sp if stream is None else C.c_void_p(stream.cuda_stream)
        _lib.check(self.engine.lib.ptts_mimi_state_reset(self.handle, sp))

    def reset_row(self, row: int, stream: torch.cuda.Stream | None = None):
        """zero the streaming carries of one sequence (a new utterance joins in `row`)"""
        sp = self.engine._sp if stream is None else C.c_void_p(stream.cuda_stream)
        _lib.check(self.engine.lib.ptts_mimi_state_reset_row(self.handle, row, sp))

    def set_pcm_i16(self, buf: torch.Tensor | None):
        """int16 copy of the PCM written by the decodes / graph captures issued after this call (None: off)"""
        _lib.check(self.engine.lib.ptts_mimi_set_pcm_i16(self.handle, _ptr(buf) if buf is not None else None))

    def _set_stage(self, kind, stage, out: torch.Tensor | None = None, mid: torch.Tensor | None = None):
        """The decodes / graph captures issued after this call run `stage`, an output stage of the class `kind`, behind the
        codec's last kernel, at its place in the chain resampler -> stretcher -> pitcher -> toner -> compressor ->
        normaliser -> leveler -> encoder (`output_chain.py`; the C side is `kind._attach` of include/ptts.h).  It writes `out`: [B, its output width],
        float32 or int16, device or pinned host; float32 on the device for the toner, the compressor and the normaliser, which a leveler
        must follow; uint8 [B, en.pitch] for the encoder.  `mid` None: it reads the frame's PCM, which must then be a DEVICE
        tensor.  Otherwise it reads the float32 device tensor `mid` [B, its input width], which the caller has given the
        stage before it as its `out`; that stage must be set on this state already, so stages are set in chain order.  A
        resampler is always first and has no `mid`.  The packer, behind the encoder, reads the uint8 device tensor the
        encoder writes and writes uint8 [B, pk.pitch].  `stage` None: off, the launches are those of before."""
        args = [None, None, None]
        if stage is not None:
            stage._check_written(out)
            if mid is not None:
                stage._check_in(mid)
            args = [stage.handle, _ptr(mid), _ptr(out)]
        if kind is Resampler:
            del args[1]
        if kind._i16:
            args.append(int(stage is not None and out.dtype == torch.int16))
        _lib.check(getattr(self.engine.lib, kind._attach)(self.handle, *args))

    def set_resampler(self, rs: "Resampler | None", out: torch.Tensor | None = None):
        self._set_stage(Resampler, rs, out)

    def set_stretcher(self, ts: "Stretcher | None", out: torch.Tensor | None = None, mid: torch.Tensor | None = None):
        self._set_stage(Stretcher, ts, out, mid)

    def set_pitcher(self, ps: "Pitcher | None", out: torch.Tensor | None = None, mid: torch.Tensor | None = None):
        self._set_stage(Pitcher, ps, out, mid)

    def set_tone(self, tn: "Toner | None", out: torch.Tensor | None = None, mid: torch.Tensor | None = None):
        self._set_stage(Toner, tn, out, mid)

    def set_dynamics(self, dy: "Dynamics | None", out: torch.Tensor | None = None, mid: torch.Tensor | None = None):
        self._set_stage(Dynamics, dy, out, mid)

    def set_loudnorm(self, ln: "Normalizer | None", out: torch.Tensor | None = None, mid: torch.Tensor | None = None):
        self._set_stage(Normalizer, ln, out, mid)

    def set_leveler(self, lv: "Leveler | None", out: torch.Tensor | None = None, mid: torch.Tensor | None = None):
        self._set_stage(Leveler, lv, out, mid)

    def set_encoder(self, en: "Encoder | None", out: torch.Tensor | None = None, mid: torch.Tensor | None = None):
        self._set_stage(Encoder, en, out, mid)

    def set_packer(self, pk: "Packer | None", out: torch.Tensor | None = None, mid: torch.Tensor | None = None):
        """`mid`: the uint8 device tensor [B, en.pitch] that the encoder on this state writes; `out`: uint8 [B, pk.pitch]"""
        self._set_stage(Packer, pk, out, mid)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Stage:
    """What the output stages share.  A subclass names itself (`_name`, in error texts; `_field`, the request field it
    serves) and its C ABI functions: `_destroy`, `_attach` (its ptts_mimi_set_*, `MimiState._set_stage`) and `_drain` (its
    set_row_drain, None for a stage without a drain flag, which `Route.drain_stage` calls `_drain_name`).  `_i16`: it
    writes float32 or int16, so those functions take is_i16; otherwise `_check_written` says what it writes.  It gives the
    widths of its lines (`_in_width`, `_out_width`), in `_row_args(row)` what `set_row` last dealt the row according to its
    host mirror, and in `_route_args(route)` what `set_row` deals a row on that `output_chain.Route`."""

    _name = _field = _destroy = _attach = _drain = _drain_name = None
    _i16 = True

    def __init__(self, engine: "Engine", batch: int):
        self.engine, self.batch = engine, batch
        self.handle = None

    def _create(self, create, *args):
        """`create(engine, *args, &handle)`; the stage then counts among the engine's states"""
        h = C.c_void_p()
        _lib.check(create(self.engine.handle, *args, C.byref(h)))
        self.handle = h
        self.engine._states.add(self)

    def _sp(self, stream):
        return self.engine._sp if stream is None else C.c_void_p(stream.cuda_stream)

    def reset(self, stream: torch.cuda.Stream | None = None):
        """every row's state back to zero (new utterances); the rows keep what `set_row` dealt them"""
        for b in range(self.batch):
            self.set_row(b, *self._row_args(b), stream)

    def _check_out(self, out):
        shape = [self.batch, self._out_width]
        if out is None or out.dtype not in (torch.float32, torch.int16) or list(out.shape) != shape or not out.is_contiguous():
            raise ValueError(f"{self._name} output: expected a contiguous float32 or int16 {shape} tensor")

    def _check_in(self, x):
        dev, shape = self.engine.device, [self.batch, self._in_width]
        if x is None or x.device != dev or x.dtype != torch.float32 or list(x.shape) != shape or not x.is_contiguous():
            raise ValueError(f"{self._name} input: expected a contiguous float32 {shape} tensor on {dev}")

    _check_written = _check_out  # what checks the tensor the stage writes

    def set_row_drain(self, row: int, on: bool = True, stream: torch.cuda.Stream | None = None):
        """from now on (stream-ordered) the row's incoming frames count as zeros"""
        if self._drain is None:
            raise AttributeError(f"the {self._name} has no drain flag")
        _lib.check(getattr(self.engine.lib, self._drain)(self.handle, int(row), int(bool(on)), self._sp(stream)))

    def _frame(self, fn, x, out, stream, *extra):
        """`fn(handle, x, out, [is_i16,] *extra, stream)` on `stream`, or on the engine's stream ordered against torch's
        current one"""
        e = self.engine
        if stream is None:
            e._pre()
        i16 = (int(out.dtype == torch.int16),) if self._i16 else ()
        _lib.check(fn(self.handle, _ptr(x), _ptr(out), *i16, *map(_ptr, extra), self._sp(stream)))
        if stream is None:
            for t in (x, out, *extra):
                if t is not None and t.is_cuda:
                    t.record_stream(e.stream)
            e._post()

    def close(self):
        if self.handle is not None:
            getattr(self.engine.lib, self._destroy)(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Stretcher(_Stage):
    """Speaking rates of `batch` sequences (include/ptts.h: ptts_stretcher; contract and plan rule: `stretch.py`).
    `plans` is a list of `stretch.StretchPlan`; a row is dealt a plan by its index (`set_row`) and starts on plan 0.
    `frame(x, out)` turns one frame x[b, :n_in(plan of b)] into out[b, :n_out(plan of b)]; `set_row_drain` makes a row's
    incoming frames count as zeros, which flushes its tail."""

    _name, _field, _destroy, _attach = "stretcher", "speed", "ptts_stretcher_destroy", "ptts_mimi_set_stretcher"
    _drain, _drain_name = "ptts_stretcher_set_row_drain", "stretch"
    _route_args = staticmethod(lambda r: (r.stretch_plan,))

    def __init__(self, engine: "Engine", batch: int, plans):
        super().__init__(engine, batch)
        self.plans = list(plans)
        self.in_max = self._in_width = max(p.n_in for p in self.plans)
        self.out_max = self._out_width = max(p.n_out for p in self.plans)
        self.k_max = max([p.K for p in self.plans if not p.identity], default=1)
        self.row_plan = [0] * batch  # host mirror of the rows' plan indices
        n = len(self.plans)
        ints = (C.c_int32 * (5 * n))(*[v for p in self.plans for v in p.ints()])
        windows = np.concatenate([p.window.reshape(-1) for p in self.plans]).astype(np.float32)
        self._create(engine.lib.ptts_stretcher_create, batch, ints, n, windows.ctypes.data_as(C.POINTER(C.c_float)),
                     windows.size)

    def n_out(self, plan_index: int) -> int:
        """output samples per frame on `plans[plan_index]`"""
        return self.plans[plan_index].n_out

    def _row_args(self, row):
        return (self.row_plan[row],)

    def set_row(self, row: int, plan_index: int, stream: torch.cuda.Stream | None = None):
        """a new sequence joins `row` on `plans[plan_index]` with a zero state, not draining; stream-ordered"""
        _lib.check(self.engine.lib.ptts_stretcher_set_row(self.handle, int(row), int(plan_index), self._sp(stream)))
        self.row_plan[row] = int(plan_index)

    def frame(self, x: torch.Tensor, out: torch.Tensor, delta: torch.Tensor | None = None,
              stream: torch.cuda.Stream | None = None):
        """x f32[B, in_max] on the device -> out (float32 or int16 [B, out_max], device or pinned host); `delta` (int32
        [B, k_max] on the device) receives the hops' deltas of the rows that are not on an identity plan"""
        e = self.engine
        self._check_in(x)
        self._check_out(out)
        if delta is not None and (delta.device != e.device or delta.dtype != torch.int32 or not delta.is_contiguous()
                                  or tuple(delta.shape) != (self.batch, self.k_max)):
            raise ValueError(f"stretcher deltas: expected a contiguous int32 [{self.batch}, {self.k_max}] tensor on {e.device}")
        self._frame(e.lib.ptts_stretch_frame, x, out, stream, delta)


class Pitcher(_Stage):
    """Pitches of `batch` sequences (include/ptts.h: ptts_pitcher; contract and plan rule: `pitch.py`).  `plans` is a list
    of `pitch.PitchPlan`; a row is dealt a plan by its index (`set_row`) and starts on plan 0.  `frame(x, out)` turns one
    frame x[b, :n(plan of b)] into out[b, :n(plan of b)], every frequency moved by the plan's ratio, `preroll` samples late;
    `set_row_drain` makes a row's incoming frames count as zeros, which flushes its tail."""

    _name, _field, _destroy, _attach = "pitcher", "pitch", "ptts_pitcher_destroy", "ptts_mimi_set_pitcher"
    _drain, _drain_name = "ptts_pitcher_set_row_drain", "pitch"
    _route_args = staticmethod(lambda r: (r.pitch_plan,))

    def __init__(self, engine: "Engine", batch: int, plans):
        super().__init__(engine, batch)
        self.plans = list(plans)
        self.width = self.in_max = self.out_max = self._in_width = self._out_width = max(p.n for p in self.plans)
        self.k_max = max([p.K for p in self.plans if not p.identity], default=1)
        self.mid_max = max([p.n_mid for p in self.plans if not p.identity], default=1)
        self.row_plan = [0] * batch  # host mirror of the rows' plan indices
        n = len(self.plans)
        ints = (C.c_int32 * (8 * n))(*[v for p in self.plans for v in p.ints()])
        windows = np.concatenate([p.sp.window.reshape(-1) for p in self.plans]).astype(np.float32)
        tables = np.concatenate([p.table.reshape(-1) for p in self.plans]).astype(np.float32)
        self._create(engine.lib.ptts_pitcher_create, batch, ints, n, windows.ctypes.data_as(C.POINTER(C.c_float)),
                     windows.size, tables.ctypes.data_as(C.POINTER(C.c_float)), tables.size)

    def _row_args(self, row):
        return (self.row_plan[row],)

    def set_row(self, row: int, plan_index: int, stream: torch.cuda.Stream | None = None):
        """a new sequence joins `row` on `plans[plan_index]` with a zero state, not draining; stream-ordered"""
        _lib.check(self.engine.lib.ptts_pitcher_set_row(self.handle, int(row), int(plan_index), self._sp(stream)))
        self.row_plan[row] = int(plan_index)

    def frame(self, x: torch.Tensor, out: torch.Tensor, delta: torch.Tensor | None = None, mid: torch.Tensor | None = None,
              stream: torch.cuda.Stream | None = None):
        """x f32[B, width] on the device -> out (float32 or int16 [B, width], device or pinned host); the test taps `delta`
        (int32 [B, k_max]) and `mid` (float32 [B, mid_max]), both on the device, receive the hops' deltas and the frame's
        mid samples of the rows that are not on an identity plan"""
        e = self.engine
        self._check_in(x)
        self._check_out(out)
        for t, dtype, w, what in ((delta, torch.int32, self.k_max, "deltas"), (mid, torch.float32, self.mid_max, "mid samples")):
            if t is not None and (t.device != e.device or t.dtype != dtype or not t.is_contiguous()
                                  or tuple(t.shape) != (self.batch, w)):
                raise ValueError(f"pitcher {what}: expected a contiguous {dtype} [{self.batch}, {w}] tensor on {e.device}")
        self._frame(e.lib.ptts_pitch_frame, x, out, stream, delta, mid)


class Leveler(_Stage):
    """Output levels of `batch` sequences (include/ptts.h: ptts_leveler; contract and plan rule: `level.py`).  `plans` is a
    list of `level.LevelPlan`; a row is dealt a plan by its index together with its gain and ceiling in dB (`set_row`;
    `gain_db` None: bypass) and starts on bypass.  `frame(x, out)` turns one frame x[b, :n(plan of b)] into
    out[b, :n(plan of b)], LA samples late; `set_row_drain` makes a row's incoming frames count as zeros, which flushes its
    tail.  A bypass row's whole line is copied.  With `true_peak` the leveler has the true-peak mode of `level.py`: a row
    dealt `true_peak=True` limits the 4x-oversampled peak, `LA + 10` samples late, and keeps a meter (`row_true_peak`); every
    other row computes what it computes on a leveler without the mode, bit for bit."""

    _name, _field, _destroy, _attach = "leveler", "level", "ptts_leveler_destroy", "ptts_mimi_set_leveler"
    _drain, _drain_name = "ptts_leveler_set_row_drain", "level"
    _route_args = staticmethod(lambda r: (*(r.level or (None, None, None)), r.true_peak))

    def __init__(self, engine: "Engine", batch: int, plans, true_peak: bool = False):
        super().__init__(engine, batch)
        self.plans = list(plans)
        self.width = self._in_width = self._out_width = max(p.n for p in self.plans)
        self.rows = [(-1, None, None)] * batch  # host mirror: (plan index, gain_db, ceiling in dB) of each row
        self.row_mode = [False] * batch         # and whether that ceiling is a true peak
        self.true_peak = bool(true_peak)
        n = len(self.plans)
        ints = (C.c_int32 * (4 * n))(*[v for p in self.plans for v in p.ints()])
        self._create(engine.lib.ptts_leveler_create, batch, ints, n)
        if self.true_peak:
            from . import level

            taps = np.ascontiguousarray(level.TP_TAPS, np.float32)
            _lib.check(engine.lib.ptts_leveler_enable_true_peak(self.handle, taps.ctypes.data_as(C.POINTER(C.c_float))))

    def _row_args(self, row):
        return (*self.rows[row], self.row_mode[row])

    def set_row(self, row: int, plan_index: int | None = None, gain_db=None, peak_dbfs=None, true_peak: bool = False,
                stream: torch.cuda.Stream | None = None):
        """a new sequence joins `row` on `plans[plan_index]` at `gain_db` under `peak_dbfs` (default -1) with a zero state,
        not draining; `gain_db` None: the row bypasses the stage.  `true_peak`: the ceiling is a true peak (dBTP), the row
        runs in true-peak mode with its meter at 0; ValueError on a leveler without the mode, on bypass and for a plan
        with LA + 10 > n.  Stream-ordered"""
        from . import level

        g, c = level.check(gain_db, peak_dbfs)
        if g is None:
            if true_peak:
                raise ValueError("a true-peak ceiling is only meaningful together with gain_db")
            idx, G, Cc = -1, 1.0, 1.0
        else:
            idx, G, Cc = int(plan_index), float(level.linear(g)), float(level.linear(c))
            if not 0 <= idx < len(self.plans):
                raise ValueError(f"leveler plan index {plan_index!r} out of range")
        if true_peak:
            if not self.true_peak:
                raise ValueError("this leveler has no true-peak mode (build it with true_peak=True)")
            p = self.plans[idx]
            level.plan(p.rate, p.n, True)  # the rule LA + 10 <= n, in its own words
            fn = self.engine.lib.ptts_leveler_set_row_tp
        else:
            fn = self.engine.lib.ptts_leveler_set_row
        _lib.check(fn(self.handle, int(row), idx, G, Cc, self._sp(stream)))
        self.rows[row], self.row_mode[row] = (idx, g, c), bool(true_peak)

    def row_true_peak(self, row: int, stream: torch.cuda.Stream | None = None):
        """the meter of `row` after every frame enqueued so far (on `stream`, or on the engine's stream): the largest
        magnitude of the 4x-oversampled output since `set_row`, linear, what `level.true_peak` reads on the samples the row
        wrote.  None for a row that is not in true-peak mode.  Waits for the stream"""
        if not self.true_peak:
            raise ValueError("this leveler has no true-peak mode (build it with true_peak=True)")
        if not 0 <= int(row) < self.batch:
            raise ValueError(f"leveler row {row!r} out of range")
        if not self.row_mode[row]:
            return None
        v = C.c_float()
        if stream is None:
            self.engine._pre()
        _lib.check(self.engine.lib.ptts_leveler_row_true_peak(self.handle, int(row), C.byref(v), self._sp(stream)))
        return float(v.value)

    def frame(self, x: torch.Tensor, out: torch.Tensor, stream: torch.cuda.Stream | None = None):
        """x f32[B, width] on the device -> out (float32 or int16 [B, width], device or pinned host)"""
        self._check_in(x)
        self._check_out(out)
        self._frame(self.engine.lib.ptts_level_frame, x, out, stream)


class Normalizer(_Stage):
    """Loudness targets of `batch` sequences (include/ptts.h: ptts_loudnorm; contract and plan rule: `loudness.py`).
    `plans` is a list of `loudness.LoudPlan`; a row is dealt a plan by its index together with its target in LUFS
    (`set_row`; `loudness_lufs` None: bypass) and starts on bypass.  `frame(x, out)` turns one frame x[b, :n(plan of b)]
    into out[b, :n(plan of b)], D = 400 ms late, under the gain that brings the row's running BS.1770 loudness to its
    target; `set_row_drain` makes a row's incoming frames count as zeros, which flushes its tail.  A bypass row's whole line
    is copied.  The output is always float32 on the device: the stage is never the last one."""

    _name, _field, _destroy, _attach = "normaliser", "loudness", "ptts_loudnorm_destroy", "ptts_mimi_set_loudnorm"
    _drain, _drain_name = "ptts_loudnorm_set_row_drain", "loud"
    _i16, _check_written = False, _Stage._check_in
    _route_args = staticmethod(lambda r: r.loud or (None, None))

    def __init__(self, engine: "Engine", batch: int, plans):
        super().__init__(engine, batch)
        self.plans = list(plans)
        self.width = self.in_max = self.out_max = self._in_width = self._out_width = max(p.n for p in self.plans)
        self.rows = [(-1, None)] * batch  # host mirror: (plan index, loudness_lufs) of each row
        n = len(self.plans)
        ints = (C.c_int32 * (2 * n))(*[v for p in self.plans for v in p.ints()])
        doubles = np.ascontiguousarray(np.concatenate([p.doubles() for p in self.plans]), dtype=np.float64)
        self._create(engine.lib.ptts_loudnorm_create, batch, ints, n, doubles.ctypes.data_as(C.POINTER(C.c_double)),
                     doubles.size)

    def _row_args(self, row):
        return self.rows[row]

    def set_row(self, row: int, plan_index: int | None = None, loudness_lufs=None, stream: torch.cuda.Stream | None = None):
        """a new sequence joins `row` on `plans[plan_index]` with the target `loudness_lufs` and a zero state, not draining;
        `loudness_lufs` None: the row bypasses the stage.  Stream-ordered"""
        from . import loudness

        t = loudness.check(loudness_lufs)
        if t is None:
            idx, t_arg = -1, 0.0
        else:
            idx, t_arg = int(plan_index), t
            if not 0 <= idx < len(self.plans):
                raise ValueError(f"normaliser plan index {plan_index!r} out of range")
        _lib.check(self.engine.lib.ptts_loudnorm_set_row(self.handle, int(row), idx, t_arg, self._sp(stream)))
        self.rows[row] = (idx, t)

    def frame(self, x: torch.Tensor, out: torch.Tensor, tap: torch.Tensor | None = None,
              stream: torch.cuda.Stream | None = None):
        """x f32[B, width] -> out f32[B, width], both on the device and distinct; the test tap `tap` (float64 [B, 4] on the
        device) receives each normalising row's completed sub-blocks, last L (NaN while undefined), last c and last Z"""
        e = self.engine
        self._check_in(x)
        self._check_in(out)
        if tap is not None and (tap.device != e.device or tap.dtype != torch.float64 or not tap.is_contiguous()
                                or tuple(tap.shape) != (self.batch, 4)):
            raise ValueError(f"normaliser tap: expected a contiguous float64 [{self.batch}, 4] tensor on {e.device}")
        self._frame(e.lib.ptts_loudnorm_frame, x, out, stream, tap)


class Encoder(_Stage):
    """Output encodings of `batch` sequences (include/ptts.h: ptts_encoder; contract: `encoding.py`).  A row is dealt its
    number of samples `n` (1 <= n <= `width`) and the name of its encoding (`set_row`) and starts as (`width`,
    "pcm_s16le").  `frame(x, out)` turns one frame x[b, :n] into the first n * bytes_per_sample bytes of out[b], a uint8
    [batch, `pitch`] tensor with `pitch` = `encoding.pitch(width)`, and writes nothing behind them.  The stage has no state
    and no drain flag."""

    _name, _field, _destroy, _attach = "encoder", "encoding", "ptts_encoder_destroy", "ptts_mimi_set_encoder"
    _i16 = False
    _route_args = staticmethod(lambda r: (r.n_out, r.encoding))

    def __init__(self, engine: "Engine", batch: int, width: int):
        from . import encoding

        super().__init__(engine, batch)
        self.width = self.in_max = self._in_width = int(width)
        self.pitch = self._out_width = encoding.pitch(self.width)  # in bytes: what a packer behind it reads
        self.rows = [(self.width, encoding.DEFAULT)] * batch  # host mirror: (n, encoding) of each row
        self._create(engine.lib.ptts_encoder_create, batch, self.width)

    def _row_args(self, row):
        return self.rows[row]

    def _check_bytes(self, out):
        shape = [self.batch, self.pitch]
        if out is None or out.dtype != torch.uint8 or list(out.shape) != shape or not out.is_contiguous():
            raise ValueError(f"{self._name} output: expected a contiguous uint8 {shape} tensor")
        if not out.is_cuda and not out.is_pinned():
            raise ValueError(f"{self._name} output: a host tensor must be pinned")

    _check_written = _check_bytes

    def set_row(self, row: int, n: int, encoding: str | None = None, stream: torch.cuda.Stream | None = None):
        """`row` holds `n` samples in `encoding` (None: "pcm_s16le") from now on.  Stream-ordered"""
        from . import encoding as rule

        name = rule.check(encoding)
        _lib.check(self.engine.lib.ptts_encoder_set_row(self.handle, int(row), int(n), rule.CODE[name], self._sp(stream)))
        self.rows[row] = (int(n), name)

    def frame(self, x: torch.Tensor, out: torch.Tensor, stream: torch.cuda.Stream | None = None):
        """x f32[B, width] on the device -> out u8[B, pitch], device or pinned host"""
        self._check_in(x)
        self._check_bytes(out)
        self._frame(self.engine.lib.ptts_encode_frame, x, out, stream)


class Packer(_Stage):
    """Output compression of `batch` sequences (include/ptts.h: ptts_flac; contract: `flac.py`), the stage behind the
    encoder.  A row is dealt its number of samples `n`, its encoding and its compression (`set_row`) and starts as
    pass-through (`width`, "pcm_s16le").  `frame(x, out)` turns the encoder's bytes x, uint8 [batch, `in_pitch`] on the
    device, into ring lines out, uint8 [batch, `pitch`] with `pitch` = `flac.pitch(width)`: the prefix {u32 nbytes, 0, 0,
    0}, then a pass-through row's n * bytes_per_sample bytes or a flac row's frame, and nothing behind 16 + nbytes rounded
    up to 16.  A flac row keeps a line counter and its previous line on the device; it has no drain flag."""

    _name, _field, _destroy, _attach = "packer", "compression", "ptts_flac_destroy", "ptts_mimi_set_packer"
    _i16 = False
    _route_args = staticmethod(lambda r: (r.n_out, r.encoding, r.compression, r.preroll, 0, r.rate))

    def __init__(self, engine: "Engine", batch: int, width: int):
        from . import encoding, flac

        super().__init__(engine, batch)
        self.width = int(width)
        self.in_pitch = self._in_width = encoding.pitch(self.width)
        self.pitch = self._out_width = flac.pitch(self.width)
        self.rows = [(self.width, encoding.DEFAULT, None, 0, 0, None)] * batch  # host mirror: what set_row took
        self._create(engine.lib.ptts_flac_create, batch, self.width)

    def _row_args(self, row):
        return self.rows[row]

    def _check_in(self, x):
        dev, shape = self.engine.device, [self.batch, self.in_pitch]
        if x is None or x.device != dev or x.dtype != torch.uint8 or list(x.shape) != shape or not x.is_contiguous():
            raise ValueError(f"{self._name} input: expected a contiguous uint8 {shape} tensor on {dev}")

    def _check_bytes(self, out):
        shape = [self.batch, self.pitch]
        if out is None or out.dtype != torch.uint8 or list(out.shape) != shape or not out.is_contiguous():
            raise ValueError(f"{self._name} output: expected a contiguous uint8 {shape} tensor")
        if not out.is_cuda and not out.is_pinned():
            raise ValueError(f"{self._name} output: a host tensor must be pinned")

    _check_written = _check_bytes

    def set_row(self, row: int, n: int, encoding: str | None = None, compression: str | None = None, preroll: int = 0,
                first_block: int = 0, rate: int | None = None, stream: torch.cuda.Stream | None = None):
        """`row` holds `n` samples in `encoding` (None: "pcm_s16le") from now on, its line counter at 0.  `compression`
        None: its bytes pass through.  "flac": its lines leave as FLAC frames at `rate` Hz, numbered from `first_block`,
        cut `preroll` samples into its sequence (`flac.py`, "the cut").  Stream-ordered"""
        from . import encoding as rule
        from . import flac

        name = rule.check(encoding)
        if flac.check(compression) is None:
            args = (0, int(n), rule.BYTES_PER_SAMPLE[name], 0, 0, 0)
        else:
            if rate is None:
                raise ValueError("packer: a flac row needs its rate")
            flac.plan(rate, n, name)
            args = (1, int(n), 2, int(rate), int(preroll), int(first_block))
        _lib.check(self.engine.lib.ptts_flac_set_row(self.handle, int(row), *args, self._sp(stream)))
        self.rows[row] = (int(n), name, compression, int(preroll), int(first_block), rate)

    def frame(self, x: torch.Tensor, out: torch.Tensor, stream: torch.cuda.Stream | None = None):
        """x u8[B, in_pitch] on the device (an encoder's output) -> out u8[B, pitch], device or pinned host"""
        self._check_in(x)
        self._check_bytes(out)
        self._frame(self.engine.lib.ptts_flac_frame, x, out, stream)


class _FilterStage(_Stage):
    """What the toner and the compressor share: float32 lines of one width in and out on the device, plans of
    `_plan_ints` ints and some doubles each, and rows that start on bypass.  A subclass names its `_create_fn`, `_set_row_fn`
    and `_frame_fn` of the C ABI."""

    _i16, _check_written = False, _Stage._check_in
    _plan_ints = _create_fn = _set_row_fn = _frame_fn = None

    def __init__(self, engine: "Engine", batch: int, plans, width: int | None = None):
        super().__init__(engine, batch)
        self.plans = list(plans)
        self.width = max(p.n for p in self.plans) if width is None else int(width)
        self.in_max = self.out_max = self._in_width = self._out_width = self.width
        self.row_plan = [-1] * batch  # host mirror of the rows' plan indices
        n = len(self.plans)
        ints = (C.c_int32 * (self._plan_ints * n))(*[v for p in self.plans for v in p.ints()])
        doubles = np.ascontiguousarray(np.concatenate([p.doubles() for p in self.plans]), dtype=np.float64)
        self._create(getattr(engine.lib, self._create_fn), batch, self.width, ints, n,
                     doubles.ctypes.data_as(C.POINTER(C.c_double)), doubles.size)

    def _row_args(self, row):
        return (self.row_plan[row],)

    def set_row(self, row: int, plan_index: int | None = None, stream: torch.cuda.Stream | None = None):
        """a new sequence joins `row` on `plans[plan_index]` with a zero state; None or -1: the row bypasses the stage.
        Stream-ordered"""
        idx = -1 if plan_index is None else int(plan_index)
        if not -1 <= idx < len(self.plans):
            raise ValueError(f"{self._name} plan index {plan_index!r} out of range")
        _lib.check(getattr(self.engine.lib, self._set_row_fn)(self.handle, int(row), idx, self._sp(stream)))
        self.row_plan[row] = idx

    def frame(self, x: torch.Tensor, out: torch.Tensor, stream: torch.cuda.Stream | None = None):
        """x f32[B, width] -> out f32[B, width], both on the device and distinct"""
        self._check_in(x)
        self._check_in(out)
        self._frame(getattr(self.engine.lib, self._frame_fn), x, out, stream)


class Toner(_FilterStage):
    """Tones of `batch` sequences (include/ptts.h: ptts_tone; contract, grammar and plan rule: `tone.py`).  `plans` is a list
    of `tone.TonePlan`; a row is dealt a plan by its index (`set_row`; None: bypass) and starts on bypass.  `frame(x, out)`
    turns one frame x[b, :n(plan of b)] into out[b, :n(plan of b)] through the plan's cascade of biquad sections, with no
    lag; the sections' states are carried from frame to frame.  A bypass row's whole line is copied.  `width` is the line's
    width, the largest n of the plans where it is left out.  The output is always float32 on the device: the stage is never
    the last one."""

    _name, _field, _destroy, _attach = "toner", "tone", "ptts_tone_destroy", "ptts_mimi_set_tone"
    _plan_ints, _create_fn, _set_row_fn, _frame_fn = 3, "ptts_tone_create", "ptts_tone_set_row", "ptts_tone_frame"
    _route_args = staticmethod(lambda r: (r.tone_plan,))


class Dynamics(_FilterStage):
    """Dynamics of `batch` sequences (include/ptts.h: ptts_dynamics; contract, grammar and plan rule: `dynamics.py`).
    `plans` is a list of `dynamics.DynPlan`; a row is dealt a plan by its index (`set_row`; None: bypass) and starts on
    bypass.  `frame(x, out)` turns one frame x[b, :n(plan of b)] into out[b, :n(plan of b)] through the plan's compressor,
    with no lag; the detector's two values are carried from frame to frame.  A bypass row's whole line is copied.  `width`
    is the line's width, the largest n of the plans where it is left out.  The output is always float32 on the device: the
    stage is never the last one."""

    _name, _field, _destroy, _attach = "compressor", "dynamics", "ptts_dynamics_destroy", "ptts_mimi_set_dynamics"
    _plan_ints, _create_fn, _set_row_fn, _frame_fn = 2, "ptts_dynamics_create", "ptts_dynamics_set_row", "ptts_dynamics_frame"
    _route_args = staticmethod(lambda r: (r.dyn_plan,))


class Resampler(_Stage):
    """Output sample rates of `batch` sequences (include/ptts.h: ptts_resampler; filters and admission rules:
    `resample.py`).  `rates[0]` is always the codec's native rate - what a row without a rate of its own runs at - followed
    by `sample_rates`; a row is dealt a rate by its index (`index_of`).  `frame(pcm, out)` turns one codec frame into
    `out[b, :out_n(rate of b)]`; each row carries 64 input samples from frame to frame, `set_row` zeroes them.  `plans`:
    the `rate_plans` of an `output_chain.ChainTable` that has designed the rates' filters already."""

    _name, _field, _destroy, _attach = "resampler", "sample_rate", "ptts_resampler_destroy", "ptts_mimi_set_resampler"
    _route_args = staticmethod(lambda r: (r.rate_index,))

    def __init__(self, engine: "Engine", batch: int, sample_rates, plans=None):
        from .output_chain import ChainTable

        super().__init__(engine, batch)
        self.plans = plans or ChainTable(engine.sample_rate, engine.frame_samples, sample_rates).rate_plans
        self.rates = [p.rate for p in self.plans]
        self._in_width = engine.frame_samples
        self.out_max = self._out_width = max(p.out_n for p in self.plans)
        self.row_rate = [0] * batch  # host mirror of the rows' rate indices
        n = len(self.plans)
        ints = [(C.c_int32 * n)(*[getattr(p, k) for p in self.plans]) for k in ("up", "down", "taps")]
        tables = np.concatenate([p.table.reshape(-1) for p in self.plans]).astype(np.float32)
        self._create(engine.lib.ptts_resampler_create, batch, *ints, n, tables.ctypes.data_as(C.POINTER(C.c_float)),
                     tables.size)

    def index_of(self, rate) -> int:
        """the rate's index (None: 0, the native rate); ValueError for a rate that is not configured"""
        from .output_chain import rate_index

        return rate_index(self.rates, rate)

    def out_n(self, rate_index: int) -> int:
        """output samples per frame at `rates[rate_index]`"""
        return self.plans[rate_index].out_n

    def _row_args(self, row):
        return (self.row_rate[row],)

    def set_row(self, row: int, rate_index: int, stream: torch.cuda.Stream | None = None):
        """a new sequence joins `row` at `rates[rate_index]` with a zero history; stream-ordered"""
        _lib.check(self.engine.lib.ptts_resampler_set_row(self.handle, int(row), int(rate_index), self._sp(stream)))
        self.row_rate[row] = int(rate_index)

    def frame(self, pcm: torch.Tensor, out: torch.Tensor, stream: torch.cuda.Stream | None = None):
        """pcm f32[B, frame_samples] on the device -> out (float32 or int16 [B, out_max], device or pinned host)"""
        self._check_in(pcm)
        self._check_out(out)
        self._frame(self.engine.lib.ptts_resample_frame, pcm, out, stream)


class Engine:
    """Weights of one model on one GPU + entry points of the hot path."""

    # PTTS_QUANT_* / PTTS_CODEC_BF16 / PTTS_CODEC_FP8 / PTTS_LM_BF16 (include/ptts.h)
    QUANT_GROUPS = {"attention": 1, "ffn": 2, "codec_bf16": 4, "codec_fp8": 8, "lm_bf16": 16, "codec_split": 32}

    def __init__(self, cfg: Config, weights: dict, device: str | torch.device = "cuda:0",
                 quantize_groups: set | frozenset | None = None, _packed: str | None = None):
        """`quantize_groups`: subset of {"attention", "ffn"} (the keys of the reference's
        quantization.apply_dynamic_int8): those Linear layers of the FlowLM transformer get int8 weights; plus
        "codec_bf16": the Mimi decoder runs with bf16 weights / activations and fp32 accumulation; "codec_fp8": its SEANet
        convolutions run on the fp8 MFMA (e4m3 weights + activations, the transformer as under codec_bf16); "lm_bf16": bf16
        weights and bf16-rounded activation operands for the FlowLM transformer's Linear layers (no reference counterpart
        for any of the three; BASELINE.json config #5 / SURVEY 8(f).4)."""
        self.lib = _lib.load()
        self.handle = None
        self._states = weakref.WeakSet()
        self._tuned = set()
        self.cfg = cfg
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("pocket_tts_amd runs on a ROCm GPU only (device must be cuda:N)")
        torch.cuda.set_device(self.device)
        h = C.c_void_p()
        if _packed is not None:
            # a packed engine: the device images come from the file, `weights` holds only what stays on the Python side
            self.has_voice_encoder = bool(weights.get("_has_voice_encoder", True))
            self.quantize_groups = frozenset(quantize_groups or ())
            _lib.check(self.lib.ptts_create_from_file(str(_packed).encode(), self.device.index or 0, C.byref(h)))
        else:
            spec = state_dict_spec(cfg)
            optional = set(mimi_encode_spec(cfg))  # checkpoints without voice cloning may lack the encoder
            if any(n not in weights for n in optional):
                spec = {k: v for k, v in spec.items() if k not in optional}
            self.has_voice_encoder = all(n in weights for n in optional)
            keep, arr = [], (_lib.PttsTensor * len(spec))()
            for i, (name, shape) in enumerate(spec.items()):
                if name not in weights:
                    raise KeyError(f"checkpoint is missing tensor {name}")
                w = weights[name]
                if isinstance(w, np.ndarray):
                    w = torch.from_numpy(w)
                if tuple(w.shape) != tuple(shape):
                    raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(w.shape)}")
                w = w.to(self.device, torch.float32).contiguous()
                keep.append(w)
                arr[i].name = name.encode()
                arr[i].d_data = w.data_ptr()
                arr[i].numel = w.numel()
            torch.cuda.synchronize(self.device)
            pc = make_ptts_config(cfg)
            flags = 0
            for g in quantize_groups or ():
                if g not in self.QUANT_GROUPS:
                    raise ValueError(f"unknown quantization group {g!r} (this build supports {sorted(self.QUANT_GROUPS)})")
                flags |= self.QUANT_GROUPS[g]
            self.quantize_groups = frozenset(quantize_groups or ())
            _lib.check(self.lib.ptts_create_ex(C.byref(pc), arr, len(spec), self.device.index or 0, flags, C.byref(h)))
            del keep
        self.handle = h
        # All work is queued on a torch-owned stream passed through the ABI's `stream` argument, so torch's
        # caching allocator (record_stream) and the library agree on one stream whose lifetime torch manages.
        self.stream = torch.cuda.Stream(device=self.device, priority=int(os.environ.get("PTTS_PRIO_LM", "0")))
        self._sp = C.c_void_p(self.stream.cuda_stream)
        t = cfg.flow_lm.transformer
        self.D, self.H, self.L = t.d_model, t.num_heads, t.num_layers
        self.ldim = cfg.mimi.quantizer.dimension
        self.frame_samples = cfg.frame_samples
        self.sample_rate = int(cfg.mimi.sample_rate)
        # embedding table + voice-path parameters stay as torch tensors (gather / prefill inputs)
        self.embed = torch.as_tensor(weights["flow_lm.conditioner.embed.weight"]).to(self.device, torch.float32)
        self.bos_before_voice = None
        if "flow_lm.bos_before_voice" in weights:
            self.bos_before_voice = torch.as_tensor(weights["flow_lm.bos_before_voice"]).to(self.device, torch.float32)

    # ---- packed-engine files (offline packer): device images + the few tensors the Python side keeps + the config
    def save_packed(self, path):
        """Writes `<path>` (device images, C ABI `ptts_engine_save`), `<path>.aux.safetensors` (embedding table,
        bos_before_voice) and `<path>.yaml` (model config + weight format).  Load with `Engine.from_packed`."""
        import safetensors.torch
        import yaml

        from .config import config_to_dict

        _lib.check(self.lib.ptts_engine_save(self.handle, str(path).encode()))
        aux = {"flow_lm.conditioner.embed.weight": self.embed.cpu().contiguous()}
        if self.bos_before_voice is not None:
            aux["flow_lm.bos_before_voice"] = self.bos_before_voice.cpu().contiguous()
        safetensors.torch.save_file(aux, str(path) + ".aux.safetensors")
        with open(str(path) + ".yaml", "w") as f:
            yaml.safe_dump(dict(config=config_to_dict(self.cfg), quantize_groups=sorted(self.quantize_groups),
                                has_voice_encoder=bool(self.has_voice_encoder)), f)

    @classmethod
    def from_packed(cls, path, device: str | torch.device = "cuda:0") -> "Engine":
        """Engine from the files `save_packed` wrote: no checkpoint, no packing, no quantisation pass."""
        import safetensors.torch
        import yaml

        from .config import config_from_dict

        meta = yaml.safe_load(open(str(path) + ".yaml"))
        aux = safetensors.torch.load_file(str(path) + ".aux.safetensors")
        aux["_has_voice_encoder"] = meta["has_voice_encoder"]
        return cls(config_from_dict(meta["config"]), aux, device, quantize_groups=set(meta["quantize_groups"]), _packed=str(path))

    # ---- stream ordering between torch's current stream and the engine stream
    def _pre(self):
        """engine stream waits for work already queued on torch's current stream (inputs)"""
        self.stream.wait_stream(torch.cuda.current_stream(self.device))

    def _post(self):
        """torch's current stream waits for the engine stream (outputs)"""
        torch.cuda.current_stream(self.device).wait_stream(self.stream)

    # ---- utilities
    def set_option(self, key: str, value: int):
        """engine options of include/ptts.h (`flow_cluster`, ...); applies to later steps / captures"""
        _lib.check(self.lib.ptts_set_option(self.handle, key.encode(), int(value)))

    def sync(self):
        _lib.check(self.lib.ptts_sync(self.handle, self._sp))

    @property
    def stream_ptr(self):
        return self.stream.cuda_stream

    def timer_start(self):
        _lib.check(self.lib.ptts_timer_start(self.handle, self._sp))

    def timer_stop_ms(self) -> float:
        ms = C.c_float()
        _lib.check(self.lib.ptts_timer_stop_ms(self.handle, self._sp, C.byref(ms)))
        return ms.value

    def tune(self, batch: int, force: bool = False) -> str:
        """Measure the tile configuration of every GEMM on the step path for this batch size (once per
        engine and batch; `PTTS_NO_TUNE=1` keeps the static heuristic).  Returns the tuner's log.

        `PTTS_TUNE_CACHE=<file>`: tile choices measured by an earlier process are imported first (a deployment,
        or a profiling run whose counters would perturb the timings, reuses them).  The tuner then still runs:
        it only measures GEMM shapes ABSENT from the table (another model, batch or weight format), so a cache
        never silently leaves shapes on the heuristic.  Newly measured shapes are appended to
        `PTTS_TUNE_CACHE_OUT` (default: the cache file itself).  Files carry the table-format version."""
        if os.environ.get("PTTS_NO_TUNE") == "1" or (batch in self._tuned and not force):
            return ""
        ver = int(self.lib.ptts_tune_version())
        head = f"# ptts-tune-version {ver}\n"
        cache = os.environ.get("PTTS_TUNE_CACHE")
        out = os.environ.get("PTTS_TUNE_CACHE_OUT", cache)
        if cache and os.path.exists(cache) and not force:
            text = open(cache).read()
            if text.startswith(head):
                self.lib.ptts_tune_import(self.handle, text.encode())
        before = self._tune_table()
        self._pre()
        _lib.check(self.lib.ptts_tune(self.handle, int(batch), self._sp))
        if batch == 1:
            # streaming path: the text prefill of a chunk sits on the first-chunk latency; its GEMM shapes depend on
            # ceil(tokens / 16) only (chunks hold <= 50 tokens + padding)
            for t in (16, 32, 48, 64):
                _lib.check(self.lib.ptts_tune_prefill(self.handle, 1, t, self._sp))
        elif os.environ.get("PTTS_TUNE_PREFILL_TOKENS"):
            # batched prefill (a group of requests with one token count): GEMMs of batch x ceil(tokens / 16) row tiles
            for t in os.environ["PTTS_TUNE_PREFILL_TOKENS"].split(","):
                _lib.check(self.lib.ptts_tune_prefill(self.handle, int(batch), int(t), self._sp))
        self._tuned.add(batch)
        after = self._tune_table()
        new = [ln for ln in after if ln not in before]
        if out and new:
            t = self.cfg.flow_lm.transformer
            fresh = not os.path.exists(out) or not open(out).read().startswith(head)
            with open(out, "w" if fresh else "a") as f:
                if fresh:
                    f.write(head)
                f.write(f"# batch {int(batch)} d_model {t.d_model} layers {t.num_layers} "
                        f"quant {'+'.join(sorted(self.quantize_groups)) or 'none'}\n" + "\n".join(new) + "\n")
        return (self.lib.ptts_tune_log(self.handle) or b"").decode()

    def streams_overlap(self, a, b) -> bool:
        """do two torch streams execute concurrently (False: the runtime mapped them to one hardware queue)"""
        return int(_lib.check(self.lib.ptts_streams_overlap(self.handle, C.c_void_p(a.cuda_stream), C.c_void_p(b.cuda_stream)))) == 1

    def concurrent_stream(self, other, tries: int = 8):
        """a stream that runs CONCURRENTLY with `other`.  HIP assigns streams round-robin to a few hardware queues
        (GPU_MAX_HW_QUEUES, default 4); a FlowLM / codec stream pair that shares a queue serialises the pipeline
        (0.88 -> 1.15 ms per step at batch 64), so the pair is checked and another stream taken if it collides."""
        prio = int(os.environ.get("PTTS_PRIO_CODEC", "0"))
        held = []  # rejected streams stay alive until the choice is made, so the round-robin moves on
        for _ in range(tries):
            s = torch.cuda.Stream(device=self.device, priority=prio)
            if self.streams_overlap(other, s):
                return s
            held.append(s)
        return held[-1]

    def _tune_table(self) -> list:
        buf = C.create_string_buffer(1 << 20)
        n = self.lib.ptts_tune_export(self.handle, buf, len(buf))
        _lib.check(int(n))
        return [ln for ln in buf.value.decode().splitlines() if ln.strip()]

    def tune_import(self, text: str) -> int:
        """Set tile choices from table lines in `_tune_table`'s format (13 key integers, then the configuration); later
        launches of those shapes use them where the configuration is admitted for the shape.  Returns the lines taken."""
        return int(_lib.check(self.lib.ptts_tune_import(self.handle, text.encode())))

    def tune_clear(self):
        """Forget every tile choice, measured or imported: launches are back on the static heuristic until `tune` runs"""
        self.lib.ptts_tune_clear(self.handle)
        self._tuned.clear()

    def profile_start(self):
        _lib.check(self.lib.ptts_profile_start(self.handle))

    def profile_stop(self) -> list:
        """-> [{site, kernel, count, total_ms, bytes, flops}] in launch order"""
        buf = C.create_string_buffer(1 << 20)
        n = self.lib.ptts_profile_stop(self.handle, buf, len(buf))
        _lib.check(int(n))
        rows = []
        for line in buf.value.decode().splitlines():
            site, kernel, cnt, ms, by, fl = line.split()
            rows.append(dict(site=site, kernel=kernel, count=int(float(cnt)), total_ms=float(ms),
                             bytes=float(by), flops=float(fl)))
        return rows

    def lm_weight_bytes(self) -> int:
        return self.lib.ptts_lm_weight_bytes(self.handle)

    def mimi_weight_bytes(self) -> int:
        return self.lib.ptts_mimi_weight_bytes(self.handle)

    def new_lm_state(self, batch: int, t_cap: int) -> LMState:
        return LMState(self, batch, t_cap)

    def new_mimi_state(self, batch: int) -> MimiState:
        return MimiState(self, batch)

    def new_resampler(self, batch: int, sample_rates) -> Resampler:
        return Resampler(self, batch, sample_rates)

    def new_stretcher(self, batch: int, plans) -> Stretcher:
        return Stretcher(self, batch, plans)

    def new_pitcher(self, batch: int, plans) -> Pitcher:
        return Pitcher(self, batch, plans)

    def new_leveler(self, batch: int, plans, true_peak: bool = False) -> Leveler:
        return Leveler(self, batch, plans, true_peak)

    def new_normalizer(self, batch: int, plans) -> Normalizer:
        return Normalizer(self, batch, plans)

    def new_toner(self, batch: int, plans, width: int | None = None) -> Toner:
        return Toner(self, batch, plans, width)

    def new_dynamics(self, batch: int, plans, width: int | None = None) -> Dynamics:
        return Dynamics(self, batch, plans, width)

    def new_encoder(self, batch: int, width: int) -> Encoder:
        return Encoder(self, batch, width)

    def new_packer(self, batch: int, width: int) -> Packer:
        return Packer(self, batch, width)

    # ---- FlowLM
    def embed_text(self, tokens: torch.Tensor) -> torch.Tensor:
        """`LUTConditioner._get_condition` gather (reference text.py:74-76); prefill input only.  tokens: int64 [B, T]
        (host or device); ids are validated where they are cheap to read, the gather itself is `ptts_embed_tokens`."""
        tokens = tokens.to(torch.int64)
        if tokens.device.type == "cpu" and tokens.numel() and (int(tokens.min()) < 0 or int(tokens.max()) >= self.embed.shape[0]):
            raise IndexError("index out of range in self")  # torch.nn.Embedding's message (reference LUT conditioner)
        tok = tokens.to(self.device).contiguous()
        out = torch.empty((*tok.shape, self.D), dtype=torch.float32, device=self.device)
        self._pre()
        _lib.check(self.lib.ptts_embed_tokens(self.handle, _ptr(self.embed), int(self.embed.shape[0]), _ptr(tok), tok.numel(),
                                              _ptr(out), self._sp))
        tok.record_stream(self.stream)
        out.record_stream(self.stream)
        self._post()
        return out

    def lm_prefill(self, state: LMState, emb: torch.Tensor, lengths=None):
        """emb f32[B, T, D]: text embeddings or voice conditioning (reference tts_model.py:722-725,899).  `lengths` (one
        int in [0, T] per row): ragged prefill - only the first lengths[b] positions of row b are real, each row ends as
        if prefilled alone with its own length and whatever the rest of `emb` holds is ignored (include/ptts.h)."""
        emb = emb.to(self.device, torch.float32).contiguous()
        if emb.dim() != 3 or emb.shape[0] != state.batch or emb.shape[2] != self.D:
            raise ValueError(f"prefill expects [B={state.batch}, T, {self.D}], got {tuple(emb.shape)}")
        self._pre()
        if lengths is None:
            _lib.check(self.lib.ptts_lm_prefill(self.handle, state.handle, _ptr(emb), emb.shape[1], self._sp))
        else:
            if len(lengths) != state.batch:
                raise ValueError(f"prefill expects one length per row ({state.batch}), got {len(lengths)}")
            h_len = (C.c_int32 * state.batch)(*[int(n) for n in lengths])
            _lib.check(self.lib.ptts_lm_prefill_ragged(self.handle, state.handle, _ptr(emb), h_len, emb.shape[1], self._sp))
        emb.record_stream(self.stream)
        self._post()

    def prefill_group(self, voices, tokens) -> LMState:
        """One group state whose row i is voice i's sequence followed by `tokens[i]`: `voices` = one (batch-1 LMState,
        its length) per row, any mix of voices and token counts.  Rows of one voice borrow its keys (KvPrefix), the text
        of all rows runs through the layers in ONE (ragged) pass.  The caller deals the rows out with `copy_row_from` and
        closes the state once those copies have run."""
        ids, lengths = pad_token_rows(tokens)
        if len(voices) != len(lengths):
            raise ValueError("need one voice per token row")
        grp = self.new_lm_state(len(lengths), max(t + n for (_, t), n in zip(voices, lengths)))
        try:
            if all(v[0] is voices[0][0] for v in voices):
                grp.copy_from(voices[0][0])  # one voice: one clone launch for all rows (what the per-row copies add up to)
            else:
                for i, v in enumerate(voices):
                    grp.copy_row_from(i, v[0], 0)
            # equal lengths need no padding: the plain entry point, launch for launch
            self.lm_prefill(grp, self.embed_text(ids), None if min(lengths) == ids.shape[1] else lengths)
        except Exception:
            grp.close()
            raise
        return grp

    def lm_decode_step(self, state: LMState, latent_in=None, noise=None, lsd_steps: int = 1,
                       eos_threshold: float = -4.0, out_latent=None, out_logit=None, out_eos=None):
        """One autoregressive step (reference tts_model.py:758-760, flow_lm.py:96-139).  Asynchronous on
        the engine stream; outputs are device tensors (allocated if not given)."""
        B = state.batch
        dev = self.device
        out_latent = torch.empty((B, self.ldim), dtype=torch.float32, device=dev) if out_latent is None else out_latent
        out_logit = torch.empty((B,), dtype=torch.float32, device=dev) if out_logit is None else out_logit
        out_eos = torch.empty((B,), dtype=torch.uint8, device=dev) if out_eos is None else out_eos
        self._pre()
        _lib.check(self.lib.ptts_lm_decode_step(
            self.handle, state.handle, _ptr(latent_in), _ptr(noise), lsd_steps, eos_threshold,
            _ptr(out_latent), _ptr(out_logit), _ptr(out_eos), self._sp))
        for t in (latent_in, noise, out_latent, out_logit, out_eos):
            if t is not None:
                t.record_stream(self.stream)
        self._post()
        return out_latent, out_logit, out_eos

    def lm_latent(self, state: LMState) -> int:
        return self.lib.ptts_lm_latent_ptr(state.handle)

    def capture_lm_step(self, state: LMState, noise, lsd_steps, eos_threshold, out_latent, out_logit, out_eos):
        g = C.c_void_p()
        _lib.check(self.lib.ptts_graph_capture_lm_step(
            self.handle, state.handle, _ptr(noise), lsd_steps, eos_threshold, _ptr(out_latent), _ptr(out_logit),
            _ptr(out_eos), C.byref(g)))
        return g

    def capture_mimi(self, state: MimiState, latent, pcm: torch.Tensor):
        """latent: device tensor f32[B, ldim] or a raw device pointer (e.g. `lm_latent(state)`)."""
        g = C.c_void_p()
        lp = C.c_void_p(latent) if isinstance(latent, int) else _ptr(latent)
        _lib.check(self.lib.ptts_graph_capture_mimi(self.handle, state.handle, lp, _ptr(pcm), C.byref(g)))
        return g

    def capture_mimi_tr(self, state: MimiState, latent, latent_b=None):
        """the codec transformer of one frame, or of the frame pair (latent, latent_b), as a graph of its own"""
        g = C.c_void_p()
        if latent_b is None:
            _lib.check(self.lib.ptts_graph_capture_mimi_tr(self.handle, state.handle, _ptr(latent), C.byref(g)))
        else:
            _lib.check(self.lib.ptts_graph_capture_mimi_tr_pair(self.handle, state.handle, _ptr(latent), _ptr(latent_b),
                                                                C.byref(g)))
        return g

    def capture_mimi_seanet(self, state: MimiState, pcm: torch.Tensor):
        """SEANet of the oldest frame the transformer has handed over, with the state's output stages behind it"""
        g = C.c_void_p()
        _lib.check(self.lib.ptts_graph_capture_mimi_seanet(self.handle, state.handle, _ptr(pcm), C.byref(g)))
        return g

    def mimi_decode_tr(self, state: MimiState, latent: torch.Tensor, latent_b: torch.Tensor | None = None):
        """eager `ptts_mimi_decode_tr`: the transformer part of one frame or of a frame pair"""
        self._pre()
        _lib.check(self.lib.ptts_mimi_decode_tr(self.handle, state.handle, _ptr(latent),
                                                _ptr(latent_b) if latent_b is not None else None, self._sp))
        for t in (latent, latent_b):
            if t is not None:
                t.record_stream(self.stream)
        self._post()

    def mimi_decode_seanet(self, state: MimiState, out_pcm=None) -> torch.Tensor:
        """eager `ptts_mimi_decode_seanet`: pcm f32[B, frame_samples] of the oldest frame handed over"""
        if out_pcm is None:
            out_pcm = torch.empty((state.batch, self.frame_samples), dtype=torch.float32, device=self.device)
        self._pre()
        _lib.check(self.lib.ptts_mimi_decode_seanet(self.handle, state.handle, _ptr(out_pcm), self._sp))
        out_pcm.record_stream(self.stream)
        self._post()
        return out_pcm

    def graph_launch(self, g, stream: torch.cuda.Stream | None = None):
        sp = self._sp if stream is None else C.c_void_p(stream.cuda_stream)
        _lib.check(self.lib.ptts_graph_launch(g, sp))

    def copy_to_host_async(self, host: torch.Tensor, dev: torch.Tensor, stream: torch.cuda.Stream | None = None):
        """device -> pinned host, truly asynchronous (torch's non_blocking copy_ blocks the host when the
        destination is a view of a pinned tensor on this stack)"""
        assert host.is_contiguous() and dev.is_contiguous() and host.numel() == dev.numel()
        sp = self._sp if stream is None else C.c_void_p(stream.cuda_stream)
        _lib.check(self.lib.ptts_copy_to_host_async(self.handle, C.c_void_p(host.data_ptr()), _ptr(dev),
                                                    host.numel() * host.element_size(), sp))

    def graph_destroy(self, g):
        self.lib.ptts_graph_destroy(g)

    # ---- voice-prompt encode path
    def encode_voice(self, audio: torch.Tensor):
        """audio f32[n_samples] (mono, model sample rate) -> (latent [frames, ldim], conditioning [frames, D]):
        `MimiModel.encode_to_latent` + speaker projection (reference mimi.py:96-119, tts_model.py:379-388)."""
        audio = audio.reshape(-1).to(self.device, torch.float32).contiguous()
        n = audio.numel()
        frames = -(-n // self.frame_samples)
        lat = torch.empty((frames, self.ldim), dtype=torch.float32, device=self.device)
        cond = torch.empty((frames, self.D), dtype=torch.float32, device=self.device)
        self._pre()
        nf = C.c_int32()
        _lib.check(self.lib.ptts_encode_voice(self.handle, _ptr(audio), n, _ptr(lat), _ptr(cond), C.byref(nf), self._sp))
        assert nf.value == frames
        return lat, cond

    # ---- Mimi
    def mimi_decode(self, state: MimiState, latent: torch.Tensor, out_pcm=None) -> torch.Tensor:
        """latent f32[B, ldim] (normalised FlowLM output) -> pcm f32[B, frame_samples]."""
        B = state.batch
        if out_pcm is None:
            out_pcm = torch.empty((B, self.frame_samples), dtype=torch.float32, device=self.device)
        self._pre()
        _lib.check(self.lib.ptts_mimi_decode(self.handle, state.handle, _ptr(latent), _ptr(out_pcm), self._sp))
        latent.record_stream(self.stream)
        out_pcm.record_stream(self.stream)
        self._post()
        return out_pcm

    def debug_read(self, state, name: str) -> torch.Tensor:
        is_mimi = isinstance(state, MimiState)
        cap = 64 * 1024 * 1024
        buf = torch.empty((cap,), dtype=torch.float32, device=self.device)
        self._pre()
        r, c = C.c_int32(), C.c_int32()
        n = self.lib.ptts_debug_read(self.handle, state.handle, int(is_mimi), name.encode(), _ptr(buf), cap,
                                     C.byref(r), C.byref(c), self._sp)
        _lib.check(int(n))
        self.sync()
        return buf[: r.value * c.value].view(r.value, c.value).clone()

    def debug_read_encoder(self, name: str, capacity: int = 1 << 23) -> torch.Tensor:
        """Test hook: intermediate `name` (include/ptts.h: ptts_debug_read_encoder) of the last `encode_voice` that ran with
        the engine option `debug_taps` set, as f32[rows, cols] of at most `capacity` floats"""
        r, c = C.c_int32(), C.c_int32()
        buf = torch.empty((capacity,), dtype=torch.float32, device=self.device)
        self._pre()
        n = self.lib.ptts_debug_read_encoder(self.handle, name.encode(), _ptr(buf), capacity, C.byref(r), C.byref(c), self._sp)
        _lib.check(int(n))
        self.sync()
        return buf[: r.value * c.value].view(r.value, c.value).clone()

    _GEMM_INTS = ("T", "xstride", "halo", "halo_mode", "wfmt", "pre", "epi", "act", "cfg", "krot", "lds_target")
    _GEMM_INS = ("x_prev", "bias", "ln_w", "ln_b", "prevec", "mod_shift", "mod_scale", "r", "g", "ls")

    def debug_gemm(self, x: torch.Tensor, w: torch.Tensor, *, want_weights: bool = False, **kw):
        """Test hook: one GEMM of the hot path's kernel family through the production dispatcher (ptts_debug_gemm in
        include/ptts.h).  x: [M * xstride][C] (ntaps = w.shape[2] > 1: M = rows of output), w: [N][C] or [N][C][ntaps];
        keyword arguments: the case's integer fields (cfg defaults to -1, the dispatcher's choice) and float32 device
        operands.  Returns None when no kernel exists for the combination, else a dict with y [M][N], the label, the
        configuration that ran and, with want_weights, the effective weights w_eff (and w_eff_lo) [N][ntaps * C] and the
        LayerNorm fold vectors ln_s / ln_c."""
        w3 = w if w.dim() == 3 else w.unsqueeze(2)
        N, Cin, ntaps = w3.shape
        c = _lib.PttsGemmCase()
        c.xstride, c.cfg, c.T = 1, -1, 16
        for k in self._GEMM_INTS:
            if k in kw:
                setattr(c, k, int(kw[k]))
        c.C, c.N, c.ntaps = Cin, N, ntaps
        c.M = x.shape[0] // c.xstride if ntaps > 1 else x.shape[0]
        keep = {}

        def dev(t):
            t = t.to(self.device, torch.float32).contiguous()
            keep[id(t)] = t
            return t.data_ptr()

        c.x, c.w = dev(x), dev(w3)
        for k in self._GEMM_INS:
            if kw.get(k) is not None:
                setattr(c, k, dev(kw[k]))
        out = {"y": torch.empty((c.M, N), dtype=torch.float32, device=self.device)}
        c.y = out["y"].data_ptr()
        if want_weights:
            out["w_eff"] = torch.empty((N, ntaps * Cin), dtype=torch.float32, device=self.device)
            c.w_eff = out["w_eff"].data_ptr()
            if c.wfmt == 3:
                out["w_eff_lo"] = torch.empty_like(out["w_eff"])
                c.w_eff_lo = out["w_eff_lo"].data_ptr()
            if c.pre == 3:
                out["ln_s"] = torch.empty((N,), dtype=torch.float32, device=self.device)
                out["ln_c"] = torch.empty((N,), dtype=torch.float32, device=self.device)
                c.ln_s, c.ln_c = out["ln_s"].data_ptr(), out["ln_c"].data_ptr()
        label = C.create_string_buffer(256)
        c.label = C.addressof(label)
        c.label_cap = 256
        self._pre()
        rc = _lib.check(self.lib.ptts_debug_gemm(self.handle, C.byref(c), self._sp))
        del keep
        if rc == 1:
            return None
        out["label"] = label.value.decode()
        out["cfg"] = c.cfg_used
        return out

    _CODEC_INTS = ("T", "halo", "par", "fmt", "kind", "pre", "epi", "act", "cfg", "mode", "cout", "stride", "yf8", "H", "Tq",
                   "ring", "cap")
    _CODEC_INS = ("x_prev", "bias", "ln_w", "ln_b", "r", "ls")

    def debug_codec_gemm(self, x: torch.Tensor, w: torch.Tensor, *, ntaps: int = 1, xs: float = 1.0, yinv: float = 1.0,
                         offset=None, yraw: bool = False, want_operands: bool = False, **kw):
        """Test hook: one GEMM of the reduced-precision codec (gemm_h_kernel / gemm_f8_kernel) or its last conv
        (pcm_conv_h_kernel, kind=1) through the production launchers (ptts_debug_codec_gemm in include/ptts.h).
        x: [M][C]; w: mode 0 [N][C] or [N][C][ntaps], mode 1 [C][cout][2 * stride] (ntaps 2).  Keyword arguments: the
        case's integer fields (cfg defaults to -1, the dispatcher's choice) and float32 device operands; offset: QKV
        positions per sequence.  Returns None when no kernel implements the combination, else a dict with y (and yraw,
        y_i16 for kind 1), the label, the tile that ran and, with want_operands, x_eff / xp_eff / w_eff / wscale (fp8) /
        ln_s / ln_c (pre 3) / rope (QKV)."""
        c = _lib.PttsCodecGemmCase()
        c.cfg, c.T = -1, 16
        for k in self._CODEC_INTS:
            if k in kw:
                setattr(c, k, int(kw[k]))
        M, Cin = x.shape
        if c.mode == 1:
            N, ntaps = w.shape[1] * (w.shape[2] // 2), 2
        else:
            w = w if w.dim() == 3 else w.unsqueeze(2)
            N, ntaps = w.shape[0], w.shape[2]
        c.M, c.N, c.C, c.ntaps = M, N, Cin, ntaps
        c.xs, c.yinv = float(xs), float(yinv)
        keep = {}

        def dev(t):
            t = t.to(self.device, torch.float32).contiguous()
            keep[id(t)] = t
            return t.data_ptr()

        def new(*shape):
            t = torch.empty(shape, dtype=torch.float32, device=self.device)
            keep[id(t)] = t
            return t

        c.x, c.w = dev(x), dev(w)
        for k in self._CODEC_INS:
            if kw.get(k) is not None:
                setattr(c, k, dev(kw[k]))
        if offset is not None:
            offs = (C.c_int32 * len(offset))(*[int(v) for v in offset])
            c.offset = C.addressof(offs)
        out = {}
        if c.kind == 1:
            out["y"], out["y_i16"] = new(M), new(M)
            c.y_i16 = out["y_i16"].data_ptr()
        elif c.epi == 3:
            out["y"] = new(M, N)
        elif c.epi == 6:
            out["y"] = new(M * c.stride, c.cout)
        else:
            out["y"] = new(M, N)
        c.y = out["y"].data_ptr()
        if yraw:
            out["yraw"] = new(*out["y"].shape)
            c.yraw = out["yraw"].data_ptr()
        if want_operands:
            out["x_eff"], out["xp_eff"] = new(M, Cin), new(M, Cin)
            c.x_eff, c.xp_eff = out["x_eff"].data_ptr(), out["xp_eff"].data_ptr()
            if c.kind == 0:
                out["w_eff"] = new(N, ntaps * Cin)
                c.w_eff = out["w_eff"].data_ptr()
                if c.fmt == 1:
                    out["wscale"] = new(N)
                    c.wscale = out["wscale"].data_ptr()
                if c.pre == 3:
                    out["ln_s"], out["ln_c"] = new(N), new(N)
                    c.ln_s, c.ln_c = out["ln_s"].data_ptr(), out["ln_c"].data_ptr()
                if c.epi == 3:
                    out["rope"] = new(M, 32, 2)
                    c.rope = out["rope"].data_ptr()
        label = C.create_string_buffer(256)
        c.label = C.addressof(label)
        c.label_cap = 256
        self._pre()
        rc = _lib.check(self.lib.ptts_debug_codec_gemm(self.handle, C.byref(c), self._sp))
        del keep
        if rc == 1:
            return None
        out["label"] = label.value.decode()
        out["cfg"] = c.cfg_used
        return out

    _ATTN_INTS = ("cap", "ring", "ctx", "splits", "h16", "layer", "pre_cap", "cascade", "kernel")

    def debug_attn(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, offset, *, pk=None, pv=None, pre_len=None,
                   pre_id=None, poison_k: float = 0.0, poison_v: float = 1e6, **kw):
        """Test hook: one attention launch through the production dispatcher (ptts_debug_attn in include/ptts.h).
        q [B][Tq][H][64], k / v [B][T][H][64], offset [B] (position of each row's first query); optional prefixes: pk / pv
        [n_pre][pre_T][H][64], pre_len [n_pre], pre_id [B] (-1: none).  Keyword arguments: the case's integer fields
        (cap defaults to T rounded up to 16, splits and kernel to -1).  Returns None when the forced kernel does not
        support the case, else a dict with y [B][Tq][H * 64] (f32; bf16 output widened), the label, the kernel table
        index and the splits used."""
        B, Tq, H, _ = q.shape
        T = k.shape[1]
        c = _lib.PttsAttnCase()
        c.B, c.Tq, c.H, c.T = B, Tq, H, T
        c.cap, c.splits, c.kernel, c.cascade = (T + 15) // 16 * 16, -1, -1, 0
        for key in self._ATTN_INTS:
            if key in kw:
                setattr(c, key, int(kw[key]))
        c.poison_k, c.poison_v = float(poison_k), float(poison_v)
        keep = {}

        def dev(t):
            t = t.to(self.device, torch.float32).contiguous()
            keep[id(t)] = t
            return t.data_ptr()

        def host(vals):
            a = (C.c_int32 * len(vals))(*[int(x) for x in vals])
            keep[id(a)] = a
            return C.addressof(a)

        c.q, c.k, c.v = dev(q), dev(k), dev(v)
        c.offset = host(offset)
        if pk is not None:
            c.n_pre, c.pre_T = pk.shape[0], pk.shape[1]
            c.pk, c.pv = dev(pk), dev(pv)
            c.pre_len, c.pre_id = host(pre_len), host(pre_id)
        out = {"y": torch.empty((B, Tq, H * 64), dtype=torch.float32, device=self.device)}
        c.y = out["y"].data_ptr()
        label = C.create_string_buffer(256)
        c.label = C.addressof(label)
        c.label_cap = 256
        self._pre()
        rc = _lib.check(self.lib.ptts_debug_attn(self.handle, C.byref(c), self._sp))
        del keep
        if rc == 1:
            return None
        out["label"] = label.value.decode()
        out["kernel"] = c.kernel_used
        out["splits"] = c.splits_used
        return out

    def close(self):
        """Destroys every state created from this engine, then the engine (order matters: states
        point into the engine)."""
        if self.handle is not None:
            for st in list(self._states):
                st.close()
            self.lib.ptts_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StepPipeline:
    """hipGraph-per-step driver in which the FlowLM step of frame t+1 overlaps the codec decode of frame t
    (the reference pipelines the same two stages with two CPU threads and a queue:
    tts_model.py:651-658,741-742).  Latents ping-pong between two buffers; `pcm` buffers are pinned host
    memory, so the codec's last kernel writes the samples straight over PCIe.  Two modes:

    * "events" (throughput, default for batch > 8): FlowLM graphs on stream 1, codec graphs on stream 2,
      ordered by two events per step (codec t after step t; step t+2 after codec t); the host never waits.
    * "fork": one graph per step with two parallel branches {FlowLM step t} || {Mimi decode of frame t-1}.
      Measured slower than "events" on ROCm 7.2 (the branches of a replayed graph run back to back).
    * "hostsync" (latency, small batch): the host waits for FlowLM step t-1 (it needs its EOS flag anyway,
      like the reference's `.item()` at tts_model.py:761), then launches the codec graph of frame t-1 on a
      second stream while step t is already running on the first.  No cross-stream event wait sits on the
      critical path (on this stack such waits around graph launches cost ~80 us per step, and the branches
      of a forked graph do not run concurrently).

    The options of `output_chain.ChainSpec` (`sample_rates`, `speeds`, `level`, `pitches`, `loudness`, `encodings`, `tones`,
    `compressions`, `dynamics`, `true_peak`; as keywords, or as one `spec`) configure the output chain behind the codec (`output_chain.py` gives its order; not in
    "fork" mode): the codec graphs end with its stages' launches.  `chain` holds the plan table (`chain.table`) and the
    stage objects, also here as `rs`, `ts`, `ps`, `tn`, `dy`, `ln`, `lv` and `en`.  `pcm[p]` are then DEVICE tensors and the
    samples reach the host through `out[p]`, the chain's pinned ring, int16 with `pcm_i16`, else float32:
    `out_of(frame)[b, :route.n_out]` is row b's frame, `pcm_of` / `pcm16_of` raise.  With the encoder (not with `pcm_i16`)
    `out[p]` are pinned uint8 tensors and `out_of(frame)[b, : route.n_out * route.bytes_per_sample]` are row b's bytes in
    its route's encoding; with the packer (`pk`, `compressions`) they are ring lines of `flac.pitch(width)` bytes, a 16-byte
    prefix {u32 nbytes, 0, 0, 0} and then the row's bytes or its FLAC frame (`flac.py`).  A row gets its way through the chain with `chain.set_row(row, chain.table.route(...), s2)` (codec
    stream); rows start on the native rate, speed 1.0, pitch 1.0, bypass and "pcm_s16le".  Without any option nothing
    changes: same buffers, same graph nodes.
    """

    NB_EVENTS = int(os.environ.get("PTTS_PIPE_NB", "4"))  # output-buffer ring depth of the "events" mode

    def __init__(self, eng: Engine, lm_state: LMState, mimi_state: MimiState, noise=None, lsd_steps: int = 1,
                 eos_threshold: float = -4.0, mode: str | None = None, pcm_i16: bool = False,
                 lm_stream: torch.cuda.Stream | None = None, spec=None, codec_pair: bool | None = None, flow_fold: bool | None = None,
                 **chain):
        from .output_chain import ChainSpec, OutputChain

        self.eng, self.st, self.ms = eng, lm_state, mimi_state
        B, dev = lm_state.batch, eng.device
        self.mode = mode or ("hostsync" if B <= 8 else "events")
        # frame pairs through the codec transformer ("events" mode, fp32 codec): None = PTTS_CODEC_PAIR (default 1) for
        # throughput batches (> 8 rows, where "events" is the default mode); smaller batches run for latency, and a frame
        # that waits for its partner is 80 ms late
        if codec_pair is None:
            codec_pair = os.environ.get("PTTS_CODEC_PAIR", "1") != "0" and B > 8
        self.codec_pair = bool(codec_pair) and self.mode == "events" and not (
            {"codec_bf16", "codec_fp8"} & set(eng.quantize_groups))
        # AdaLN modulations inside the flow cluster's hand-off waits (LMState.set_flow_fold): None = PTTS_FLOW_FOLD (default
        # 1) for throughput batches with an fp32 FlowLM; set on the state before its graphs are captured.  The library
        # still takes today's launches where the state does not qualify (per-row LSD capacity, flow_dim, weight format).
        if flow_fold is None:
            flow_fold = os.environ.get("PTTS_FLOW_FOLD", "1") != "0" and B > 8
        self.flow_fold = bool(flow_fold) and self.mode == "events" and not (
            {"lm_bf16", "attention", "ffn", "codec_split"} & set(eng.quantize_groups))
        # the plan table first: what the rules refuse is refused before anything is allocated
        table = ChainSpec.of(spec, **chain).table(eng.sample_rate, eng.frame_samples)
        if not table.empty and self.mode == "fork":
            raise ValueError("sample_rates / speeds / pitches / tones / dynamics / loudness / level / encodings: not available in the "
                             "'fork' mode")
        # ring of output buffers (latent -> codec input, EOS flags, PCM).  Throughput mode keeps 4 so that the FlowLM
        # stream may run up to 3 steps ahead of the codec stream (with 2 the two streams move in lock-step and every
        # hiccup of one stalls the other); the latency modes need only 2.  A host loop over the "events" mode must have
        # read flag[t % nb] / pcm[t % nb] of step t - nb before it calls step() for step t.
        self.nb = nb = self.NB_EVENTS if self.mode == "events" else 2
        self.chain = OutputChain(eng, B, table, nb, pcm_i16)
        self.out = self.chain.out
        self.rs, self.ts, self.ps, self.tn, self.dy, self.ln, self.lv, self.en = self.chain.per_kind()
        self.pk = self.chain.pk
        self.lat = [torch.zeros(B, eng.ldim, device=dev) for _ in range(nb)]
        self.logit = [torch.empty(B, device=dev) for _ in range(nb)]
        self.flag = [torch.zeros(B, dtype=torch.uint8).pin_memory() for _ in range(nb)]  # EOS flags land on the host
        # without a chain the codec's last kernel writes pinned memory; with one, device memory the first stage reads
        self.pcm = [torch.zeros(B, eng.frame_samples, device=dev) if self.out is not None else
                    torch.zeros(B, eng.frame_samples).pin_memory() for _ in range(nb)]
        self.ev = [torch.cuda.Event() for _ in range(nb)]    # codec frame (f % nb) complete -> pcm_of(f) valid
        self.ev_lm = [torch.cuda.Event() for _ in range(nb)]  # FlowLM step (t % nb) complete -> flag valid
        self.s1 = lm_stream or eng.stream  # FlowLM stream (several pipelines of one engine may use their own)
        self.s2 = eng.concurrent_stream(self.s1)
        eng.sync()
        torch.cuda.synchronize(dev)
        eng.tune(B)  # before capture: graphs freeze the tile choices
        lib, H = eng.lib, eng.handle
        if self.flow_fold:  # (never switched off here: another pipeline's graphs of this state may carry it)
            try:
                lm_state.set_flow_fold(True)
            except _lib.PttsError:  # the state already has graphs captured without it: this pipeline runs as they do
                self.flow_fold = False
        self.g_first = [eng.capture_lm_step(lm_state, noise, lsd_steps, eos_threshold, self.lat[p], self.logit[p],
                                            self.flag[p]) for p in range(nb)]
        # optional 16-bit PCM beside the fp32 one (the WAV sample format, data/audio.py:79), also pinned
        self.pcm16 = [torch.zeros(B, eng.frame_samples, dtype=torch.int16).pin_memory() for _ in range(nb)] \
            if pcm_i16 and self.out is None else None
        self.g_last, self.g_sn, self.g_tr1, self.g_tr2 = [], [], [], []
        for p in range(nb):
            if self.out is not None:  # the 16-bit conversion happens behind the last output stage
                self.chain.attach(mimi_state, p)
            else:
                mimi_state.set_pcm_i16(self.pcm16[p] if pcm_i16 else None)
            self.g_last.append(eng.capture_mimi(mimi_state, self.lat[p], self.pcm[p]))
            if self.codec_pair:  # the frame's parts: SEANet with the same stages behind it as the whole frame
                self.g_sn.append(eng.capture_mimi_seanet(mimi_state, self.pcm[p]))
                self.g_tr1.append(eng.capture_mimi_tr(mimi_state, self.lat[p]))
                self.g_tr2.append(eng.capture_mimi_tr(mimi_state, self.lat[(p - 1) % nb], self.lat[p]))
        mimi_state.set_pcm_i16(None)
        self.chain.detach(mimi_state)
        self.g_both = []
        if self.mode == "fork":
            for p in range(nb):
                g = C.c_void_p()
                _lib.check(lib.ptts_graph_capture_pipelined(
                    H, lm_state.handle, mimi_state.handle, _ptr(noise), lsd_steps, eos_threshold, _ptr(self.lat[p]),
                    _ptr(self.logit[p]), _ptr(self.flag[p]), _ptr(self.lat[p ^ 1]), _ptr(self.pcm[p ^ 1]), C.byref(g)))
                self.g_both.append(g)
        for p in range(nb):
            self.ev[p].record(self.s2)
        self.t = 0          # FlowLM steps launched for the current utterances
        self.decoded = 0    # codec frames launched

    def restart(self, routes=None, first_blocks=None):
        """new utterances: flush the pending frame, codec state back to zero carries.  `routes` (one `output_chain.Route`
        per row): the rows join the output chain on these; None: they keep theirs.  `first_blocks` (one int per row, with
        `routes`): the number of each flac row's first frame; None: 0"""
        self.flush()
        if self.mode != "fork":
            # zero carries on the CODEC stream: ordered behind the frames already queued there and ahead of the next
            # utterance's first frame, off the FlowLM stream's critical path (clone + prefill + first step)
            self.ms.reset(self.s2)
            if routes is None:
                self.chain.reset(self.s2)
            for b, route in enumerate(routes or ()):
                self.chain.set_row(b, route, self.s2, first_block=first_blocks[b] if first_blocks else 0)
        else:
            self.ms.reset()
        self.t = 0
        self.decoded = 0

    def _decode_pending(self):
        """hostsync mode: wait for FlowLM step t-1 on the host, then start its codec frame on stream 2"""
        f = self.decoded
        q = f % self.nb
        self.ev_lm[q].synchronize()
        self.eng.graph_launch(self.g_last[q], self.s2)
        self.ev[q].record(self.s2)
        self.decoded += 1
        return f

    def step(self):
        """Launch FlowLM step t and the decode of frame t-1.  Returns the index of the frame whose PCM is
        complete when `done_event(frame)` fires (None for the first step).  After the call,
        `flag[(t-1) % nb]` (hostsync mode) holds the EOS flags of step t-1.

        With `codec_pair` the codec runs behind every SECOND step: after an odd step t the transformer of the frame pair
        (t-1, t) in one launch sequence, then SEANet of t-1 and of t, each with its `done_event`; the call returns t (frame
        t-1 is complete before it).  An even step returns None and leaves its frame pending: the next step, `flush()` or
        `restart()` decodes it, and until then `done_event` of that frame is the event of an EARLIER frame."""
        eng, p = self.eng, self.t % self.nb
        done = None
        if self.mode == "fork":
            if self.decoded < self.t:
                eng.graph_launch(self.g_both[p])
                self.ev[p ^ 1].record(eng.stream)
                self.decoded += 1
                done = self.decoded - 1
            else:
                eng.graph_launch(self.g_first[p])
        elif self.mode == "events":
            self.s1.wait_event(self.ev[p])             # codec frame t-nb done: lat[p] / pcm[p] are free
            eng.graph_launch(self.g_first[p], self.s1)  # FlowLM step t -> lat[p]
            self.ev_lm[p].record(self.s1)
            if self.codec_pair and self.t % 2 == 0:
                pass  # the frame waits for its partner
            elif self.codec_pair:
                q = (p - 1) % self.nb
                self.s2.wait_event(self.ev_lm[p])           # step t done, and step t-1 before it on the same stream
                eng.graph_launch(self.g_tr2[p], self.s2)    # transformer of frames t-1 and t
                eng.graph_launch(self.g_sn[q], self.s2)     # SEANet frame t-1 -> pcm[q]
                self.ev[q].record(self.s2)
                eng.graph_launch(self.g_sn[p], self.s2)     # SEANet frame t -> pcm[p]
                self.ev[p].record(self.s2)
                self.decoded += 2
                done = self.t
            else:
                self.s2.wait_event(self.ev_lm[p])
                eng.graph_launch(self.g_last[p], self.s2)  # codec frame t -> pcm[p] (overlaps FlowLM step t+1)
                self.ev[p].record(self.s2)
                self.decoded += 1
                done = self.t
        else:
            self.s1.wait_event(self.ev[p])  # frame t-2 decoded: lat[p] / pcm[p] may be reused (long done)
            eng.graph_launch(self.g_first[p], self.s1)
            self.ev_lm[p].record(self.s1)
            if self.decoded < self.t:
                done = self._decode_pending()
        self.t += 1
        return done

    # ---- building blocks for a host-driven loop with an EOS decision per step (TTSModel) ----------
    def lm_step_async(self) -> int:
        """launch FlowLM step t on stream 1; returns t"""
        p = self.t % self.nb
        self.s1.wait_event(self.ev[p])  # frame t-2 decoded: lat[p] may be overwritten
        self.eng.graph_launch(self.g_first[p], self.s1)
        self.ev_lm[p].record(self.s1)
        self.t += 1
        return self.t - 1

    def wait_flags(self, step: int) -> torch.Tensor:
        """host waits for FlowLM step `step`; returns its EOS flags u8[B] (pinned host memory)"""
        self.ev_lm[step % self.nb].synchronize()
        return self.flag[step % self.nb]

    def decode_async(self, frame: int):
        """launch the codec decode of `frame` on stream 2 (call after wait_flags(frame))"""
        q = frame % self.nb
        self.eng.graph_launch(self.g_last[q], self.s2)
        self.ev[q].record(self.s2)
        self.decoded = frame + 1

    def flush(self):
        """decode the last pending frame (no FlowLM step rides along)"""
        if self.decoded >= self.t:
            return None
        if self.mode == "hostsync":
            return self._decode_pending()
        p = (self.t - 1) % self.nb
        if self.codec_pair:  # the frame an even step left pending, as a single frame in its two parts, on the codec stream
            self.s2.wait_event(self.ev_lm[p])
            self.eng.graph_launch(self.g_tr1[p], self.s2)
            self.eng.graph_launch(self.g_sn[p], self.s2)
            self.ev[p].record(self.s2)
            self.decoded += 1
            return self.decoded - 1
        self.eng.graph_launch(self.g_last[p])
        self.ev[p].record(self.eng.stream)
        self.decoded += 1
        return self.decoded - 1

    def pcm_of(self, frame: int) -> torch.Tensor:
        """host tensor [B, frame_samples] of `frame` (valid after `done_event(frame).synchronize()`)"""
        if self.out is not None:
            raise RuntimeError("this pipeline resamples or stretches its output: read out_of(frame)")
        return self.pcm[frame % self.nb]

    def out_of(self, frame: int) -> torch.Tensor:
        """with an output chain: host tensor [B, widest line] of `frame`, row b's samples in its first `route.n_out` entries"""
        if self.out is None:
            raise RuntimeError("this pipeline has no sample_rates: read pcm_of(frame)")
        return self.out[frame % self.nb]

    def done_event(self, frame: int):
        """event that fires when the codec decode of `frame` (PCM in `pcm_of(frame)`) is complete"""
        return self.ev[frame % self.nb]

    def pcm16_of(self, frame: int) -> torch.Tensor:
        if self.out is not None:
            raise RuntimeError("this pipeline resamples or stretches its output: read out_of(frame)")
        return self.pcm16[frame % self.nb]

    def sync(self):
        self.s1.synchronize()
        self.eng.stream.synchronize()
        self.s2.synchronize()

    def close(self):
        self.sync()
        for g in self.g_first + self.g_last + self.g_both + self.g_sn + self.g_tr1 + self.g_tr2:
            self.eng.graph_destroy(g)
        self.chain.close()
