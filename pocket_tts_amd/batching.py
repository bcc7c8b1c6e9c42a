"""Continuous batching of utterances on one GPU.

The reference serves one request at a time: `/tts` starts a thread that runs `generate_audio_stream` for that
request alone (main.py:80-181) and the model is "not thread safe" (tts_model.py:491-492).  Here a fixed set of
SLOTS shares one batched FlowLM state and one batched codec state; the hipGraphs of the step are captured
once.  A request JOINS a free slot (its voice state + text are prefilled on a batch-1 state and copied into the
slot's row, the slot's codec carries are zeroed), is decoded in lock-step with the other slots with its own
position, EOS bookkeeping and frame count (tts_model.py:756-768 per row), and LEAVES when its loop would
break; the slot is then parked until the next request arrives.  Chunks reach the caller as they are decoded:
fp32 `[frame_samples]` tensors or, with `pcm_format="i16"`, the 16-bit samples of the WAV stream written by
the codec's last kernel (data/audio.py:79).

With temp == 0 every request reproduces `TTSModel.generate_audio` for the same text and voice (same frame
count, waveform equal up to fp32 summation order: batch tiles differ from batch-1 tiles).

A request may bring its own temperature, noise clamp and EOS threshold (a server's per-request settings): they are
written to its slot's row of the batch state (`LMState.set_row_sampling`) before the row's first step, and the step's
kernels read them per row.  A request without any of them runs exactly as the model's settings would.

A request may also bring a `seed`: its slot's row then draws from the request's own stream (`LMState.set_row_seed`, one
row seed per text chunk from `engine.chunk_seed`), so the noise of the request does not depend on the slot it was dealt,
on the step at which it joined or on the other requests, and equals what `TTSModel.generate_audio(..., seed=)` draws.

A batcher built with options of `output_chain.ChainSpec` lets a request choose its way through the output chain with the
fields of `ChainTable.route`: the codec graphs end with the chain's stages (`output_chain.py` gives their order and what each
does), each slot's row runs on its request's `Route`, and `Request.sample_rate` / `Request.encoding` tell the consumer what
the chunks are: `route.n_out` samples a frame, fp32, or with the encoder typed views of the row's bytes (int16, float32, or
uint8 for G.711).  Samples stay the unit of every count.

The stretcher, the pitcher, the normaliser and the leveler lag, so their rows are "rows whose output chain lags" (the drain
rule of `output_chain.py`): a request of F frames delivers exactly F * n_out samples, the scheduler drops the row's pre-roll,
the sum of its stages' pre-rolls, sets the row to drain at its first lagging stage before the first codec frame past the
request's last one is queued, and holds the slot for ceil(pre-roll / n_out) drain frames.  To know that frame in time it reads
the EOS flags of such a row no later than `frames_after_eos` steps behind.  The resampler, the toner, the compressor and the
encoder do not lag: the toner and the compressor have a state but no drain flag, the zeros of a draining row ring out through
them, and a toned or compressed row lags by the limiter behind it like a levelled one.  The normaliser's measurement restarts with every text chunk, so the chunks of a long
request are normalised one by one.

The chunks of a long text are independent (each starts from the voice state), so with `parallel_chunks` = W a request runs up
to W of them at a time in rows of their own (`submit`), and `chunk_order.ChunkOrder` hands their audio to the consumer in text
order.  `submit_script` makes one request of segments with different voices, and `Request.cancel` takes a request out of
`waiting` and out of its slots (`_purge`, which a failed request's siblings, `_fail` and `close` go through as well).
"""

from __future__ import annotations

import collections
import logging
import math
import numbers
import queue
import threading

import torch

from .text import estimate_max_gen_len, prepare_text_prompt, split_into_best_sentences

logger = logging.getLogger(__name__)


def eos_bookkeeping(local_step: int, max_gen_len: int, frames_after_eos: int, eos_step, flag: bool):
    """Per-row restatement of the reference's generation loop (tts_model.py:756-775), evaluated after FlowLM step
    `local_step` (0-based) of an utterance: returns `(eos_step, n_emit)`.  `n_emit` is None while the row keeps
    running; otherwise it is the number of frames the utterance consists of: the latent of the step at which the
    reference's loop breaks is NOT decoded, and without EOS the row stops after `max_gen_len` frames."""
    if local_step >= max_gen_len:
        return eos_step, max_gen_len
    if flag and eos_step is None:
        eos_step = local_step
    if eos_step is not None and local_step >= eos_step + frames_after_eos:
        return eos_step, local_step
    return eos_step, None


def eos_bookkeeping_rows(local_step, max_gen_len, frames_after_eos, eos_step, n_emit, flags, rows=None):
    """`eos_bookkeeping` for many rows at once, in place on the int arrays `eos_step` / `n_emit` (-1 = None).
    `local_step`: scalar or array (rows of a continuous batch are at different steps of their utterances); rows whose
    `n_emit` is already decided, or that `rows` (bool mask) excludes, are left alone."""
    import numpy as np

    run = n_emit < 0
    if rows is not None:
        run = run & rows
    ls = np.broadcast_to(np.asarray(local_step), n_emit.shape)
    maxed = run & (ls >= max_gen_len)
    n_emit[maxed] = np.broadcast_to(max_gen_len, n_emit.shape)[maxed]
    run = run & ~maxed
    first = run & flags & (eos_step < 0)
    eos_step[first] = ls[first]
    done = run & (eos_step >= 0) & (ls >= eos_step + frames_after_eos)
    n_emit[done] = ls[done]


def check_parallel_chunks(value, bound: int | None = None) -> int:
    """`value` as the number of text chunks of one request that may wait or own slots at a time: an integer >= 1, and
    <= `bound` where one is given; ValueError otherwise (bool and float are refused)"""
    if isinstance(value, bool) or not isinstance(value, numbers.Integral) or int(value) < 1:
        raise ValueError(f"parallel_chunks must be an integer >= 1, got {value!r}")
    if bound is not None and int(value) > bound:
        raise ValueError(f"parallel_chunks must be in [1, {bound}] (the batcher's own), got {value!r}")
    return int(value)


_FRAME = object()  # through a request's chunk order: one codec frame of the chunk has been delivered (`Request.frames`)


class Request:
    """One submitted text.  Iterate to receive chunks; `result()` waits for the whole waveform."""

    def __init__(self, rid: int, sample_rate: int | None = None, encoding: str | None = None,
                 compression: str | None = None):
        self.id = rid
        self.sample_rate = sample_rate  # rate of the chunks (the codec's own unless the request asked for another)
        self.encoding = encoding        # encoding of the chunks (None: the batcher's one sample format)
        self.compression = compression  # "flac": each chunk is one whole FLAC frame as a uint8 tensor (`flac.py`)
        self.blocks = 0                 # FLAC frames delivered so far: the number of the next one
        # a request with `peak_dbtp`: the largest reading of its rows' true-peak meters over the text chunks that have
        # finished, linear (`level.true_peak` of what they delivered); None for a request without the mode
        self.true_peak: float | None = None
        self._q: queue.Queue = queue.Queue()
        self.frames = 0
        self.error: Exception | None = None
        self._pending_chunks = 0  # text chunks not yet finished
        self._batcher = None      # the batcher that runs the request (`cancel`)
        # a request with several chunks in flight: its `chunk_order.ChunkOrder`, which forwards to `_forward`.  None: one
        # chunk at a time, whose items go to `_q` directly
        self._order = None

    def _forward(self, item):
        """what the chunk order emits, in text order: a frame tick, an item for the consumer, or the final None.  `frames`
        and `blocks` therefore count what has been forwarded, and a FLAC frame, numbered from 0 within its chunk by its
        row, gets its number in the request's stream here (`flac.renumber`)"""
        if item is _FRAME:
            self.frames += 1
            return
        if item is not None and self.compression is not None:
            from .flac import renumber

            item = torch.frombuffer(bytearray(renumber(item.numpy().tobytes(), self.blocks)), dtype=torch.uint8)
            self.blocks += 1
        self._q.put(item)

    @property
    def true_peak_dbtp(self) -> float | None:
        """`true_peak` in dBTP (-inf for digital silence); None for a request without `peak_dbtp`"""
        if self.true_peak is None:
            return None
        return 20.0 * math.log10(self.true_peak) if self.true_peak > 0 else -math.inf

    def cancel(self):
        """Ends the request: callable from any thread, takes effect at the scheduler's next iteration.  Its chunks leave
        `waiting` and their slots, the consumer's iteration ends without an error behind what had been forwarded, and
        `result()` returns that.  A second call, or a call after the request's end, does nothing."""
        if self._batcher is not None:
            self._batcher._cancel(self)

    def __iter__(self):
        while True:
            item = self._q.get()
            if item is None:
                if self.error is not None:
                    raise self.error
                return
            yield item

    def iter_batches(self):
        """Like iterating, but each item is the list of every chunk that has arrived by then (at least one): a consumer
        that hands chunks to another thread or an event loop pays that hand-off once per batch, not once per frame."""
        while True:
            items = [self._q.get()]
            while items[-1] is not None:
                try:
                    items.append(self._q.get_nowait())
                except queue.Empty:
                    break
            done = items[-1] is None  # the sentinel is always the last item of a request
            if done:
                items.pop()
            if items:
                yield items
            if done:
                if self.error is not None:
                    raise self.error
                return

    def result(self) -> torch.Tensor:
        parts = list(self)
        if not parts:
            return torch.zeros(0)
        return torch.cat(parts)


class _Job:
    """one text chunk of a request while it owns a slot"""

    __slots__ = ("req", "tokens", "voice", "gen", "fae", "start", "last", "samp", "lsd", "seed", "route", "index")

    def __init__(self, req, tokens, voice, gen, fae, last, samp=None, lsd=None, seed=None, route=None, index=0):
        self.req, self.tokens, self.voice, self.gen, self.fae, self.last = req, tokens, voice, gen, fae, last
        self.index = index     # which of the request's text chunks this is
        self.route = route     # the request's way through the pipeline's output chain (`output_chain.Route`)
        self.seed = seed       # the chunk's row seed (engine.chunk_seed of the request's seed), or None: the state's stream
        self.samp = samp       # (temperature, noise_clamp, eos_threshold) of the request, or None: the model's settings
        self.lsd = lsd         # the request's lsd_decode_steps, or None: the model's
        self.start = None      # global step of its first FlowLM step


class ContinuousBatcher:
    def __init__(self, model, slots: int = 16, capacity: int = 1024, pcm_format: str = "f32", noise_seed: int = 0,
                 max_lsd_decode_steps: int | None = None, spec=None, parallel_chunks: int = 1, **chain):
        """`capacity`: KV positions per slot (voice + text + generated frames of one chunk must fit).

        `parallel_chunks` = W: up to W text chunks of one request wait or own slots at a time (`submit`); it is the default
        and the upper bound of a request's own value.  1: the chunks of a request run one after the other, as before.

        The options of `output_chain.ChainSpec` (`sample_rates`, `speeds`, `level`, `pitches`, `loudness`, `encodings`,
        `tones`, `compressions`, `dynamics`, `true_peak`; as keywords, or as one `spec`) let each request choose its way through the output chain with the fields of
        `ChainTable.route` (`submit`).  `encodings` needs `pcm_format` left at its default (ValueError).  Without any of them
        every request gets the codec's samples in `pcm_format`, with the same graphs and buffers as before.

        `max_lsd_decode_steps` = K lets each request choose its own `lsd_decode_steps` in [1, K] (`submit`).  A step then
        takes as long as its slowest group of 16 rows.  None: every request runs the model's `lsd_decode_steps`, with the
        same graphs as before.

        The scheduler never waits for the GPU on the step path: FlowLM step g and codec frame g are queued on the two
        streams of the "events" pipeline, and the EOS flags / PCM of a step are read from pinned memory `lag` <= nb steps
        later (as soon as the frame's event has fired).  A row therefore runs up to nb steps past the end of its
        utterance before its slot is parked (those frames are dropped); frame counts and waveforms are exactly those of
        the reference's loop (tts_model.py:756-768 per row)."""
        import numpy as np

        from .engine import StepPipeline
        from .output_chain import ChainSpec

        self.parallel_chunks = check_parallel_chunks(parallel_chunks)  # before anything is allocated
        spec = ChainSpec.of(spec, **chain)
        if pcm_format not in ("f32", "i16"):
            raise ValueError("pcm_format must be 'f32' or 'i16'")
        if (spec.encodings is not None or spec.compressions is not None) and pcm_format != "f32":
            raise ValueError("pcm_format and encodings exclude each other: with encodings a request asks for 'pcm_s16le' "
                             "or 'pcm_f32le' itself")
        self.model, self.eng, self.B = model, model.engine, slots
        self.capacity, self.pcm_format = capacity, pcm_format
        eng = self.eng
        # what the chain's rules refuse is refused before anything is allocated
        spec.table(eng.sample_rate, eng.frame_samples)
        self.st = eng.new_lm_state(slots, capacity)
        self.ms = eng.new_mimi_state(slots)
        # also at temp 0 (std 0: no draws): the seed is the one rows overridden to a temperature > 0 draw with
        self.st.set_noise(model.temp, noise_seed)
        for b in range(slots):
            self.st.set_row_active(b, False)
        if max_lsd_decode_steps is not None:
            k = int(max_lsd_decode_steps)
            if k != max_lsd_decode_steps or not 1 <= k <= 64:
                raise ValueError(f"max_lsd_decode_steps must be an integer in [1, 64], got {max_lsd_decode_steps}")
            self.st.reserve_row_lsd(k)  # before the pipeline captures its graphs
        self.max_lsd = max_lsd_decode_steps
        self.pipe = StepPipeline(eng, self.st, self.ms, None, model.lsd_decode_steps, float(model.eos_threshold),
                                 mode="events", pcm_i16=(pcm_format == "i16"), spec=spec,
                                 codec_pair=False)  # rows are reset between any two frames: single frames
        self.chain = self.pipe.chain
        self.rs, self.ts, self.ps, self.tn, self.dy, self.ln, self.lv, self.en = self.chain.per_kind()
        self.pk = self.chain.pk  # with the packer a ring line begins with a prefix that says how many bytes follow
        # the output chain has a stage that may lag
        self.lagging = self.ts is not None or self.ps is not None or self.lv is not None
        self.pipe.restart()
        self.slot: list = [None] * slots                 # running _Job per slot
        # per-slot bookkeeping of the job that owns the slot (arrays: one numpy pass per step instead of a Python loop)
        self.a_start = np.zeros(slots, np.int64)
        self.a_gen = np.zeros(slots, np.int64)
        self.a_fae = np.zeros(slots, np.int64)
        self.a_eos = np.full(slots, -1, np.int64)
        self.a_emit = np.full(slots, 0, np.int64)         # >= 0: no running job in the slot
        self.row_samp = [False] * slots                   # the slot's row carries a sampling override
        self.row_lsd = [False] * slots                    # ... an lsd_decode_steps override
        self.row_seed = [False] * slots                   # ... a seed
        # rows whose output chain lags (`speeds`, `level`): output samples the slot's job has produced, whether its row has
        # been set to drain,
        # and the global frame after which a job that has ended leaves its slot (-1: not ended)
        self.a_pos = np.zeros(slots, np.int64)
        self.row_drain = [False] * slots
        self.a_release = np.full(slots, -1, np.int64)
        self.a_blocks = np.zeros(slots, np.int64)  # FLAC frames the slot's job has delivered
        # held by the background scheduler around each iteration: other users of the engine (e.g. a voice-prompt encode
        # on a request thread) take it to run between the scheduler's steps (`exclusive`)
        self.engine_lock = threading.RLock()
        self.waiting: collections.deque = collections.deque()
        self.g = 0            # global step counter == pipe.t
        self.collected = 0    # frames [0, collected) have been read (EOS flags) and routed (PCM)
        self._next_id = 0
        self._lock = threading.Lock()
        self._wake = threading.Condition(self._lock)
        self._thread = None
        self._stop = False
        self._chain: dict = {}  # request id -> deque of follow-up chunks (released as the request's earlier chunks leave)
        self._cancels: list = []  # requests whose `cancel` waits for the scheduler's next iteration
        self._outstanding: dict = {}  # request id -> Request, from submit() until its final sentinel: what _fail / stop notify
        self._failed: Exception | None = None
        self._closed = False

    # ---- submission (any thread) ---------------------------------------------------------------
    def submit(self, model_state: dict, text: str, frames_after_eos: int | None = None, max_tokens: int = 50,
               temperature: float | None = None, noise_clamp: float | None = None,
               eos_threshold: float | None = None, lsd_decode_steps: int | None = None,
               parallel_chunks: int | None = None, seed: int | None = None, **request) -> Request:
        """Same text handling as `generate_audio_stream` (tts_model.py:618-631): long texts are split into
        chunks, each of which runs from the voice state: one after the other, or with `parallel_chunks` = W > 1 (an int in
        [1, the batcher's own]; None: the batcher's own) up to W of them at a time in rows of their own.  The first
        min(W, n) chunks wait at once, and each chunk that leaves its slot releases the next, so the request never has
        more than W chunks waiting or in slots and the other requests take the remaining slots in arrival order.  The
        consumer receives what the serial run delivers, in text order (`chunk_order.ChunkOrder`): what a later chunk
        produces early is held until the chunks before it have finished, and `Request.frames` / `Request.blocks` count
        what has been forwarded.  A FLAC row of such a request numbers its frames from 0 and the host renumbers each
        frame as it is forwarded (`flac.renumber`).  The one-segment case of `submit_script`.

        `temperature`, `noise_clamp` (<= 0: none) and `eos_threshold` apply to this request only; None means the model's
        value.  A request that gives none of them runs with the model's settings exactly.  `lsd_decode_steps` (an int in
        [1, max_lsd_decode_steps]) is the number of Euler steps of this request's flow head; a batcher built without
        `max_lsd_decode_steps` accepts only the model's value.  `seed` (an int in [0, 2**63)) makes the request's noise
        reproducible: the same seed, text and settings draw the same noise in any slot, under any traffic, and in
        `TTSModel.generate_audio(..., seed=)`; None draws from the batch state's own stream.

        `**request`: the request's way through the output chain, the fields of `ChainTable.route` (`sample_rate`, `speed`,
        `gain_db`, `peak_dbfs`, `pitch`, `loudness_lufs`, `encoding`, `tone`, `compression`, `dynamics`, `peak_dbtp`), checked against the batcher's table:
        ValueError for what it refuses, TypeError for another name.  A request with `peak_dbtp` (the ceiling as a true peak)
        has its row's meter read at the end of each text chunk: `Request.true_peak` / `true_peak_dbtp`.  A request whose row lags (a speed, a pitch, a loudness
        target, a tone, a compressor setting or a gain) needs frames_after_eos >= 1."""
        return self.submit_script([(model_state, text)], frames_after_eos, max_tokens, temperature=temperature,
                                  noise_clamp=noise_clamp, eos_threshold=eos_threshold, lsd_decode_steps=lsd_decode_steps,
                                  seed=seed, parallel_chunks=parallel_chunks, **request)

    def submit_script(self, segments, frames_after_eos: int | None = None, max_tokens: int = 50,
                      temperature: float | None = None, noise_clamp: float | None = None,
                      eos_threshold: float | None = None, lsd_decode_steps: int | None = None, seed: int | None = None,
                      parallel_chunks: int | None = None, **request) -> Request:
        """One request made of `segments`, a non-empty list of `(model_state, text)` pairs: a dialogue script.  Each text is
        split as `submit` splits it, the chunks of all segments form one list in order, each chunk runs on its segment's
        voice, and chunk i of that list draws from `chunk_seed(seed, i)`.  One `Request`, one ordered stream and one route
        for all segments; every other argument is `submit`'s and applies to the whole script.  An empty text in any
        segment is the ValueError of `submit`."""
        from .engine import check_seed, chunk_seed
        from .tts_model import _state_current_end

        m = self.model
        if self._failed is not None:
            raise RuntimeError(f"the batcher has stopped after an error: {self._failed}")
        segments = list(segments)
        if not segments:
            raise ValueError("a script needs at least one segment")
        for _, text in segments:
            if not text or not text.strip():
                raise ValueError("Text to generate cannot be empty")
        window = self.parallel_chunks if parallel_chunks is None else check_parallel_chunks(parallel_chunks,
                                                                                             self.parallel_chunks)
        samp = None
        if temperature is not None or noise_clamp is not None or eos_threshold is not None:
            t = float(m.temp if temperature is None else temperature)
            c = m.noise_clamp if noise_clamp is None else noise_clamp
            c = 0.0 if c is None else float(c)
            e = float(m.eos_threshold if eos_threshold is None else eos_threshold)
            if not (math.isfinite(t) and t >= 0):
                raise ValueError(f"temperature must be a finite number >= 0, got {temperature}")
            if math.isnan(c):
                raise ValueError("noise_clamp must be a number")
            if not math.isfinite(e):
                raise ValueError(f"eos_threshold must be a finite number, got {eos_threshold}")
            samp = (t, c, e)
        if seed is not None:
            seed = check_seed(seed)
            if samp is None and m.noise_clamp is not None:
                # a seeded request draws as `generate_audio(seed=)` does: with the model's noise clamp
                samp = (float(m.temp), float(m.noise_clamp), float(m.eos_threshold))
        route = self.chain.table.route(**request)
        lsd = None
        if lsd_decode_steps is not None:
            n = lsd_decode_steps
            if isinstance(n, bool) or not isinstance(n, numbers.Integral):
                raise ValueError(f"lsd_decode_steps must be an integer, got {lsd_decode_steps!r}")
            n = int(n)
            if self.max_lsd is None:
                if n != m.lsd_decode_steps:
                    raise ValueError(f"lsd_decode_steps {n}: this batcher runs every request at {m.lsd_decode_steps} "
                                     "(build it with max_lsd_decode_steps for per-request values)")
            elif not 1 <= n <= self.max_lsd:
                raise ValueError(f"lsd_decode_steps must be in [1, {self.max_lsd}], got {n}")
            else:
                lsd = n
        chunks = []  # (voice state, its KV positions, chunk text) of every chunk of every segment, in order
        for model_state, text in segments:
            t_voice = _state_current_end(model_state)
            chunks += [(model_state, t_voice, c) for c in
                       split_into_best_sentences(m.tokenizer.encode, m.tokenizer.sp, text, max_tokens,
                                                 m.pad_with_spaces_for_short_inputs, m.remove_semicolons)]
        jobs = []
        with self._lock:
            req = Request(self._next_id, route.rate, route.encoding, route.compression)
            self._next_id += 1
        req._batcher = self
        for i, (model_state, t_voice, chunk) in enumerate(chunks):
            _, guess = prepare_text_prompt(chunk, m.pad_with_spaces_for_short_inputs, m.remove_semicolons)
            fae = frames_after_eos if frames_after_eos is not None else (
                m.model_recommended_frames_after_eos if m.model_recommended_frames_after_eos is not None else guess + 2)
            for lags, what in ((route.stretched, "a speed"), (route.pitched, "a pitch"),
                               (route.loud is not None, "a loudness target"), (route.toned, "a tone"),
                               (route.dynamic, "a compressor setting"), (route.level is not None, "a gain")):
                if lags and fae < 1:
                    raise ValueError(f"a request with {what} needs frames_after_eos >= 1: the row is set to drain before the "
                                     "frame that follows its last one is queued")
            ids = m.tokenizer.encode(chunk)
            gen = estimate_max_gen_len(len(ids), m.config.mimi.frame_rate)
            need = t_voice + len(ids) + gen + self.pipe.nb + 2  # a row runs up to nb steps past its end before it is parked
            if need > self.capacity:
                raise ValueError(f"request needs {need} KV positions; slot capacity is {self.capacity}")
            jobs.append(_Job(req, torch.tensor(ids, dtype=torch.long)[None, :], model_state, gen, fae, i == len(chunks) - 1,
                             samp, lsd, None if seed is None else chunk_seed(seed, i), route, i))
        req._pending_chunks = len(jobs)
        window = min(window, len(jobs))
        if window > 1:  # several chunks in flight: their items reach the queue through the chunk order
            from .chunk_order import ChunkOrder

            req._order = ChunkOrder(len(jobs), req._forward)
        with self._wake:
            if self._failed is not None or self._closed:
                raise RuntimeError("the batcher is closed" if self._failed is None else
                                   f"the batcher has stopped after an error: {self._failed}")
            self._outstanding[req.id] = req
            self.waiting.extend(jobs[:window])
            if len(jobs) > window:
                self._chain[req.id] = collections.deque(jobs[window:])
            self._wake.notify_all()
        return req

    def _cancel(self, req):
        """`Request.cancel`: noted here by any thread, carried out by the scheduler (`_cancel_due`)"""
        with self._wake:
            if req.id in self._outstanding and req not in self._cancels:
                self._cancels.append(req)
                self._wake.notify_all()

    # ---- scheduler (one thread) ----------------------------------------------------------------
    def _admit(self):
        """Waiting jobs join the free slots.  All jobs of one admit round, whatever their voices and token counts, are
        prefilled as ONE batch (each row's voice KV cloned from its device-resident copy, one ragged pass through the
        layers: `Engine.prefill_group`) and dealt to their slots."""
        eng = self.eng
        with self._lock:
            free = [b for b in range(self.B) if self.slot[b] is None and self.a_emit[b] >= 0]
            take = []
            while self.waiting and len(take) < len(free):
                take.append(self.waiting.popleft())
        if not take:
            return
        order: dict = {}
        for job in take:
            order.setdefault(id(job.voice), len(order))
        jobs = sorted(take, key=lambda j: order[id(j.voice)])  # rows of one voice next to each other, as they arrived
        # slots: rows of one voice share its keys (KvPrefix) and the decode attention scores a shared prefix once per 4
        # NEIGHBOURING rows (attn_cascade_kernel), so a job prefers a 4-row group that holds only its own voice
        voice_of = {b: id(self.slot[b].voice) for b in range(self.B) if self.slot[b] is not None}

        def pick(vid):
            def score(b):
                mates = [voice_of[r] for r in range(b & ~3, min(self.B, (b & ~3) + 4)) if r in voice_of]
                return (any(v != vid for v in mates), -sum(v == vid for v in mates), b)
            b = min(free, key=score)
            free.remove(b)
            voice_of[b] = vid
            return b

        try:
            self._admit_group(jobs, [pick(id(job.voice)) for job in jobs])
        except (ValueError, KeyError, IndexError, TypeError) as e:
            if len(jobs) == 1:
                # a bad request (malformed voice state, capacity): fail THIS request, keep serving the others.  The
                # job is in no list any more, so it is notified here (its consumer would block forever).
                self._end_request(jobs[0].req, e)
                return
            for job in jobs:  # find the bad one(s): admit the group's members one by one
                with self._lock:
                    if job.req.id not in self._outstanding:
                        continue  # a chunk of a request that another of its chunks has just failed
                    b = next(b for b in range(self.B) if self.slot[b] is None and self.a_emit[b] >= 0)
                try:
                    self._admit_group([job], [b])
                except (ValueError, KeyError, IndexError, TypeError) as e1:
                    self._end_request(job.req, e1)

    def _admit_group(self, jobs, rows):
        eng, model = self.eng, self.model
        voices: dict = {}  # each distinct voice once: device-resident, no host sync on a hit
        grp = None
        try:
            for job in jobs:
                if id(job.voice) not in voices:
                    voices[id(job.voice)] = model._voice_acquire(job.voice)
            grp = eng.prefill_group([voices[id(j.voice)] for j in jobs], [j.tokens for j in jobs])
            for i, b in enumerate(rows):
                self.st.copy_row_from(b, grp, i)   # KV rows, position, BOS as the pending input, row active
            for job, b in zip(jobs, rows):         # the row's sampling settings, before its first step
                if job.samp is not None:
                    self.st.set_row_sampling(b, *job.samp)
                elif self.row_samp[b]:
                    self.st.clear_row_sampling(b)
                self.row_samp[b] = job.samp is not None
                if job.lsd is not None:
                    self.st.set_row_lsd(b, job.lsd)
                elif self.row_lsd[b]:
                    self.st.clear_row_lsd(b)
                self.row_lsd[b] = job.lsd is not None
                if job.seed is not None:
                    self.st.set_row_seed(b, job.seed)
                elif self.row_seed[b]:
                    self.st.clear_row_seed(b)
                self.row_seed[b] = job.seed is not None
            eng.sync()  # the group state is freed below; its clone kernels must have run
        finally:
            if grp is not None:
                grp.close()
            for voice in voices.values():
                model._voice_release(voice)
        for job, b in zip(jobs, rows):
            # the slot's codec carries: zero on the codec stream, behind the frames already queued there
            self.ms.reset_row(b, self.pipe.s2)
            # the row's route and a zero state in every stage, same stream; a flac row numbers its frames on from what the
            # request's earlier text chunks have delivered, which is not known while they still run: a row of a request with
            # several chunks in flight numbers from 0, and the host renumbers each frame as it is forwarded
            self.chain.set_row(b, job.route, self.pipe.s2, first_block=0 if job.req._order is not None else job.req.blocks)
            self.a_blocks[b] = 0
            if self.lagging:
                self.a_pos[b], self.row_drain[b], self.a_release[b] = 0, False, -1
            job.start = self.g
            self.slot[b] = job
            self.a_start[b], self.a_gen[b], self.a_fae[b] = self.g, job.gen, job.fae
            self.a_eos[b], self.a_emit[b] = -1, -1

    def _end_request(self, req, error: Exception | None = None):
        """final sentinel of a request (with `error`: the consumer's iteration raises it); removes every chunk it still has
        anywhere (`_purge`).  Without an error this is a cancellation: the consumer's iteration ends behind what it has
        been forwarded"""
        with self._wake:
            if self._outstanding.pop(req.id, None) is None:
                return
        self._purge(req)
        if error is not None:
            req.error = error
        if req._order is not None:
            req._order.cancel()  # nothing held is forwarded any more; emits the sentinel
        else:
            req._q.put(None)

    def _purge(self, req):
        """removes every job of `req` from `waiting`, from `_chain` and from the slots.  A slot is left as a job that ends
        leaves it: the row parked, no job, nothing to emit, nothing to release or drain; the next admission resets the
        row's codec and chain state, and `_process` drops the frames of the row that are still in flight, because their
        slot is empty"""
        with self._wake:
            self._chain.pop(req.id, None)
            if any(j.req is req for j in self.waiting):
                self.waiting = collections.deque(j for j in self.waiting if j.req is not req)
        for b in range(self.B):
            job = self.slot[b]
            if job is None or job.req is not req:
                continue
            try:
                self.st.set_row_active(b, False)
            except Exception:
                if self._failed is None:  # after the scheduler's failure the row's state no longer matters
                    raise
            self.slot[b] = None
            self.a_emit[b], self.a_release[b], self.row_drain[b] = 0, -1, False

    def _cancel_due(self):
        """carries out the cancellations noted since the last iteration"""
        with self._wake:
            reqs, self._cancels = self._cancels, []
        for req in reqs:
            self._end_request(req)

    def _process(self, frame: int):
        """EOS decisions of FlowLM step `frame` and the PCM of codec frame `frame`, for every slot whose job had started
        by then; rows whose loop breaks at this step leave their slot (the break-step frame is not emitted)."""
        import numpy as np

        pipe = self.pipe
        pipe.done_event(frame).synchronize()  # codec frame done => the FlowLM step's flags are on the host too
        q = frame % pipe.nb
        rows = (self.a_emit < 0) & (self.a_start <= frame)
        held = np.nonzero(self.a_release >= 0)[0] if self.lagging else ()
        if not rows.any() and not len(held):
            return
        eos_bookkeeping_rows(frame - self.a_start, self.a_gen, self.a_fae, self.a_eos, self.a_emit,
                             pipe.flag[q].numpy() != 0, rows)
        # one copy of the frame out of the pinned ring (numpy memcpy: no intra-op thread team), rows are views of it
        if pipe.out is not None:
            ring = pipe.out_of(frame)
        else:
            ring = pipe.pcm16_of(frame) if self.pcm_format == "i16" else pipe.pcm_of(frame)
        pcm = torch.from_numpy(ring.numpy().copy())
        for b in held:  # jobs that have ended and flush their chain's tail: this is one of their drain frames
            job = self.slot[b]
            self._deliver(b, job, pcm[b])
            if frame >= self.a_release[b]:
                self.a_release[b] = -1
                self._read_meter(int(b), job)
                self.slot[b] = None
                self._finish(job)
        for b in np.nonzero(rows)[0]:
            job = self.slot[b]
            if self.a_emit[b] < 0:
                order = job.req._order  # None: one chunk at a time, straight to the queue
                if self.lagging or self.en is not None:
                    self._deliver(b, job, pcm[b])
                elif order is None:
                    job.req._q.put(pcm[b] if self.rs is None else pcm[b, :job.route.n_out])
                else:
                    order.push(job.index, pcm[b] if self.rs is None else pcm[b, :job.route.n_out])
                if order is None:
                    job.req.frames += 1
                else:
                    order.push(job.index, _FRAME)
                continue
            if self.a_eos[b] < 0:
                logger.warning("Maximum generation length reached without EOS, this very often indicates an error.")
            self.st.set_row_active(int(b), False)
            drain = job.route.drain_frames
            if drain:
                # `frame` is the first one past the job's end and, by _drain_due, the first one its row saw as zeros
                if not self.row_drain[b]:
                    raise RuntimeError("a row whose output chain lags ended before it was set to drain")
                self._deliver(b, job, pcm[b])
                if drain > 1:
                    self.a_release[b] = frame + drain - 1
                    continue
            self._read_meter(int(b), job)
            self.slot[b] = None
            self._finish(job)

    def _read_meter(self, b, job):
        """a text chunk in true-peak mode leaves slot `b`: its row's meter into the request's `true_peak`.  The frame that
        flushed its tail is done, and the frames queued behind it are zeros to a draining row, which move no meter; the
        read is ordered on the codec stream before the `set_row` of the slot's next job, and waits for that stream"""
        if job.route.true_peak:
            m = self.lv.row_true_peak(b, self.pipe.s2)
            if m is not None:
                job.req.true_peak = m if job.req.true_peak is None else max(job.req.true_peak, m)

    def _deliver(self, b, job, line):
        """routes the part of a frame of slot `b` that belongs to its job (`Route.take`): to the request's queue, or
        through its chunk order where it has several chunks in flight"""
        order = job.req._order
        put = job.req._q.put if order is None else (lambda item: order.push(job.index, item))
        if self.pk is not None:
            from .flac import PREFIX

            nbytes = int.from_bytes(line[:4].numpy().tobytes(), "little")
            line = line[PREFIX:]
            if job.route.compression is not None:
                # the kernel has cut the pre-roll: a line holds one whole frame, or nothing while the row leads; a job of
                # F frames delivers F of them
                if nbytes and (self.a_emit[b] < 0 or self.a_blocks[b] < self.a_emit[b]):
                    put(line[:nbytes])
                    self.a_blocks[b] += 1
                    if order is None:  # through the order the request counts, and numbers, what it forwards
                        job.req.blocks += 1
                return
        pos = int(self.a_pos[b])
        lo, hi = job.route.take(pos, None if self.a_emit[b] < 0 else int(self.a_emit[b]))
        if hi > lo:
            bps = job.route.bytes_per_sample
            if bps is None:
                put(line[lo:hi])
            else:  # the encoder's ring is in bytes: the job's samples as a typed view of them
                from . import encoding

                put(line[lo * bps:hi * bps].view(encoding.torch_dtype(job.route.encoding)))
        self.a_pos[b] = pos + job.route.n_out

    def _drain_due(self):
        """Before codec frame g is queued: every row whose output chain lags (a stretch, a pitch, a level) and whose job
        ends before that frame is set to drain on the codec stream, so that the frames past the job's end count as zeros:
        through the stretcher's flag where the row is stretched (what the stretcher emits past its tail is zero, which is
        what the stages behind it then read), else through the pitcher's, else through the leveler's.  A job's end is known `frames_after_eos`
        frames ahead once the EOS flags up to then have been read; where they have not, this reads them (it waits for
        the frames concerned), which a row without a speed never needs."""
        for b in range(self.B):
            job = self.slot[b]
            if job is None or self.row_drain[b] or job.route.preroll == 0:
                continue
            start, gen, fae = int(self.a_start[b]), int(self.a_gen[b]), int(self.a_fae[b])
            local = self.g - start
            while True:
                if self.a_emit[b] >= 0:
                    end = int(self.a_emit[b])
                elif self.a_eos[b] >= 0:
                    end = min(int(self.a_eos[b]) + fae, gen)
                elif local >= gen:
                    end = gen
                elif local < max(self.collected - start, 0) + fae:
                    end = None  # no EOS in the frames read so far: frame `local` belongs to the job
                else:
                    # the flags of local frame `local - fae` decide; collected <= g - fae < g here
                    self._process(self.collected)
                    self.collected += 1
                    continue
                break
            if end is not None and local >= end and self.slot[b] is job:
                self.chain.drain_row(b, job.route, self.pipe.s2)
                self.row_drain[b] = True

    def _finish(self, job):
        req = job.req
        with self._wake:
            req._pending_chunks -= 1
            nxt = self._chain.get(req.id)
            if nxt:  # the chunk that leaves releases the request's next one: its window stays full
                self.waiting.appendleft(nxt.popleft())
                if not nxt:
                    del self._chain[req.id]
            elif req._pending_chunks == 0:
                self._outstanding.pop(req.id, None)
                if req._order is None:
                    req._q.put(None)
        if req._order is not None:
            req._order.finish(job.index)  # flushes what the next chunks have produced; the sentinel behind the last chunk

    def _check_gpu_error(self):
        if self.st.error():  # synchronises the FlowLM stream: only called when idle / every 512 steps
            raise RuntimeError("libptts: a cooperative FlowLM kernel timed out; audio generated since the last check is invalid")

    def step(self) -> bool:
        """One scheduler iteration: admit, read the steps whose frames are complete, queue FlowLM step g + codec frame g.
        Returns False when there is nothing to run."""
        if self._cancels:
            self._cancel_due()
        self._admit()
        pipe, nb = self.pipe, self.pipe.nb
        # mandatory for frame g - nb (its pinned buffers are about to be reused), opportunistic for the later ones
        while self.collected < self.g and (self.g - self.collected >= nb or pipe.done_event(self.collected).query()):
            self._process(self.collected)
            self.collected += 1
        if all(j is None for j in self.slot):
            self._drain()
            return bool(self.waiting)
        if self.lagging:
            self._drain_due()
            if all(j is None for j in self.slot):
                self._drain()
                return bool(self.waiting)
        pipe.step()
        self.g += 1
        if self.g % 512 == 0:
            self._check_gpu_error()
        return True

    def _drain(self):
        """read the frames still in flight (nothing is queued behind them)"""
        while self.collected < self.g:
            self._process(self.collected)
            self.collected += 1

    def run_until_idle(self):
        while self.step():
            pass
        self._drain()
        self._check_gpu_error()

    # ---- background operation ------------------------------------------------------------------
    def start(self):
        def loop():
            torch.cuda.set_device(self.eng.device)
            while True:
                with self._wake:
                    if self._stop:
                        return
                    idle = not self.waiting and all(j is None for j in self.slot)
                try:
                    if idle:
                        if self._cancels:
                            with self.engine_lock:
                                self._cancel_due()
                        if self.collected < self.g:
                            with self.engine_lock:
                                self._drain()  # the last frames of the rows that just left; may queue a follow-up chunk
                                self._check_gpu_error()
                        with self._wake:
                            if not self._stop and not self.waiting:
                                self._wake.wait(timeout=0.05)
                    else:
                        with self.engine_lock:
                            self.step()
                except Exception as e:  # forward to every waiting consumer, like the reference's result_queue errors
                    self._fail(e)
                    return

        self._stop = False
        self._thread = threading.Thread(target=loop, daemon=True, name="ptts-batcher")
        self._thread.start()

    @property
    def failed(self) -> Exception | None:
        """the error the scheduler stopped on, or None"""
        return self._failed

    def exclusive(self, fn, *args, **kwargs):
        """runs `fn` on the calling thread while the background scheduler waits between two of its iterations (work
        that shares the engine with the scheduler, such as encoding a voice prompt)"""
        with self.engine_lock:
            return fn(*args, **kwargs)

    def _fail(self, e: Exception):
        """the scheduler cannot continue: every outstanding request - waiting, admitted or mid-admission - gets the
        error, and later submit() calls raise"""
        logger.error("batcher failed: %s", e)
        with self._wake:
            self._failed = e
            reqs = list(self._outstanding.values())
            self.waiting.clear()
        for r in reqs:
            self._end_request(r, e)

    def stop(self):
        with self._wake:
            self._stop = True
            self._wake.notify_all()
        if self._thread is not None:
            self._thread.join()
            self._thread = None

    def close(self):
        """stops the scheduler; requests still outstanding receive an error instead of blocking their consumers"""
        self.stop()
        with self._wake:
            self._closed = True
            reqs = list(self._outstanding.values())
            self.waiting.clear()
        for r in reqs:
            self._end_request(r, RuntimeError("the batcher was closed before this request finished"))
        self.pipe.sync()
        self.pipe.close()
        self.st.close()
        self.ms.close()
