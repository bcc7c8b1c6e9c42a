// The output stages' shared host code (ptts_stage.h) and the one kernel they share.
#include "ptts_stage.h"

void stage_buffer(StageBase &b, void **p, size_t bytes, const void *host) {
  if (b.er != hipSuccess) return;
  b.er = hipMalloc(p, bytes);
  if (b.er != hipSuccess) return;
  b.owned.push_back(*p);
  b.er = host ? hipMemcpy(*p, host, bytes, hipMemcpyHostToDevice) : hipMemset(*p, 0, bytes);
}

void stage_free(StageBase &b) {
  hipSetDevice(b.e->device);
  hipDeviceSynchronize();
  for (void *p : b.owned) hipFree(p);
  b.owned.clear();
}

int stage_row_ok(const StageBase *b, const char *fn, const char *noun, int row, const char *what, int index, int lowest) {
  const std::string f = std::string(fn) + ": ";
  if (!b) return fail(-1, f + "null " + noun);
  if (row < 0 || row >= b->B) return fail(-1, f + "row out of range");
  if (what && (index < lowest || index >= b->n_plans)) return fail(-1, f + what + " index out of range");
  return 0;
}

__global__ void stage_set_drain_kernel(int *row_drain, int row, int on) { row_drain[row] = on; }

int stage_set_row_drain(StageBase *b, const char *fn, const char *noun, int row, int on, void *stream) {
  CHK(stage_row_ok(b, fn, noun, row));
  StageLock lock;
  CHK(stage_enter(b->e, lock));
  stage_set_drain_kernel<<<1, 1, 0, S(b->e, stream)>>>(b->row_drain, row, on != 0);
  HIPCHK(hipGetLastError());
  return 0;
}
