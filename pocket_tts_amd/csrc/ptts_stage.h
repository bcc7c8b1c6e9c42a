// What the host sides of the nine output stages share (ptts_resample.hip .. ptts_flac.hip): the head of every ptts_<stage>
// struct, its device buffers, the refusals and the entry frame of its C ABI, and the drain flag.  The units keep their
// extern "C" definitions, their plan validation and their kernels; ptts_codec.hip's output chain reads a stage through StageBase.
#pragma once
#include "ptts_host.h"

#pragma GCC visibility push(hidden)

// Every ptts_<stage> derives from this and from nothing else, without virtual functions: a stage's address is its
// StageBase's, which is how ptts_codec.hip reads the void * of a ChainLink.
struct StageBase {
  ptts_engine *e = nullptr;
  int B = 0, n_plans = 0;
  int in_width = 0, out_width = 0;  // samples of the longest line the stage reads and writes: what the chain compares
  int *row_plan = nullptr;          // [B] the row's plan (the resampler's: rate); null: the stage has no plans
  int *row_drain = nullptr;         // [B] != 0: the row's incoming frames count as zeros; null: the stage has no such flag
  std::vector<void *> owned;        // every device buffer of the stage, and the only list stage_destroy frees from
  hipError_t er = hipSuccess;       // the first failure of stage_buffer, or of stage_finish's synchronisation
};

typedef std::unique_lock<std::recursive_mutex> StageLock;
// The engine's lock for the caller's scope, and the engine's device: the one way a stage's entry point takes them
inline int stage_enter(ptts_engine *e, StageLock &lock) {
  lock = StageLock(e->mu);
  HIPCHK(hipSetDevice(e->device));
  return 0;
}

// ---- create and destroy -----------------------------------------------------------------------------------------------
// A new T under the engine's lock, on its device
template <class T>
int stage_new(ptts_engine *e, int batch, int n_plans, int in_width, int out_width, StageLock &lock, T **st) {
  CHK(stage_enter(e, lock));
  *st = new T();
  StageBase *b = *st;
  b->e = e; b->B = batch; b->n_plans = n_plans; b->in_width = in_width; b->out_width = out_width;
  return 0;
}
// One owned device buffer of `bytes` bytes: a copy of `host`, or zeros without one.  After a failure it does nothing.
void stage_buffer(StageBase &b, void **p, size_t bytes, const void *host);
template <class T>
void stage_zeros(StageBase &b, T *&p, size_t n) { stage_buffer(b, (void **)&p, n * sizeof(T), nullptr); }
template <class T>
void stage_copy(StageBase &b, T *&p, const T *host, size_t n) { stage_buffer(b, (void **)&p, n * sizeof(T), host); }
template <class T>
void stage_fill(StageBase &b, T *&p, size_t n, T value) { stage_copy(b, p, std::vector<T>(n, value).data(), n); }
// Waits for the device, then frees what the stage owns
void stage_free(StageBase &b);
template <class T>
void stage_destroy(T *st) {
  if (!st) return;
  stage_free(*st);
  delete st;
}
// The end of a create: the one synchronisation; after any failure everything is freed and "<fn>: <HIP's words>" is the error
template <class T>
int stage_finish(T *st, T **out, const char *fn) {
  if (st->er == hipSuccess) st->er = hipDeviceSynchronize();
  if (st->er != hipSuccess) {
    const hipError_t er = st->er;
    stage_destroy(st);
    return fail(-2, std::string(fn) + ": " + hipGetErrorString(er));
  }
  *out = st;
  return 0;
}

// ---- the entry points' refusals and frames ----------------------------------------------------------------------------
// "<fn>: null <noun>", "<fn>: row out of range" and, with `what` ("plan", "rate"), "<fn>: <what> index out of range" for an
// index outside [lowest, n_plans): lowest is -1 for a stage with a bypass
int stage_row_ok(const StageBase *b, const char *fn, const char *noun, int row, const char *what = nullptr, int index = 0,
                 int lowest = 0);
// <stage>_set_row_drain, whole
int stage_set_row_drain(StageBase *b, const char *fn, const char *noun, int row, int on, void *stream);
// <stage>_frame: "<fn>: null argument" unless the stage and its buffers (args) are there, then lock, device, bind_engine and
// enqueue(stream)
template <class F>
int stage_frame(StageBase *b, bool args, const char *fn, void *stream, F enqueue) {
  if (!b || !args) return fail(-1, std::string(fn) + ": null argument");
  StageLock lock;
  CHK(stage_enter(b->e, lock));
  bind_engine(b->e);
  return enqueue(S(b->e, stream));
}

#pragma GCC visibility pop
