// C ABI of hk_replay_push / hk_replay_sample (include/hironaka_hip_replay.h, additions within ABI 6): argument
// validation and launch of hk::replay_push_kernel / hk::replay_sample_kernel.  No allocation, no synchronisation; every
// status is decided before the launch.
#include "hk_replay_kernel.h"

using namespace hk;

namespace {

// what both entry points ask of a descriptor, but for the batch side's pointers (a batch of no rows has none)
int check_desc(const hk_replay_desc* q) {
  if (!q) return HK_ERR_NULL;
  if (q->ncols < 1 || q->ncols > HK_REPLAY_MAX_COLS) return HK_ERR_SHAPE;
  if (q->capacity < 1) return HK_ERR_SHAPE;
  if (!q->cursor) return HK_ERR_NULL;
  for (int c = 0; c < q->ncols; ++c) {
    const hk_replay_col& col = q->col[c];
    if (!col.ring) return HK_ERR_NULL;
    if (col.row_bytes < 1 || col.rows_stride_bytes < col.row_bytes) return HK_ERR_SHAPE;
    if (col.row_bytes > kReplayMaxRowBytes) return HK_ERR_UNSUPPORTED;
  }
  if (!aligned(q->cursor, 8)) return HK_ERR_ALIGN;
  return HK_OK;
}

int fill_args(const hk_replay_desc* q, ReplayArgs& a) {
  for (int c = 0; c < q->ncols; ++c) {
    const hk_replay_col& col = q->col[c];
    if (!col.rows) return HK_ERR_NULL;
    ReplayCol& k = a.col[c];
    k.ring = static_cast<char*>(col.ring);
    k.rows = static_cast<char*>(col.rows);
    k.stride = col.rows_stride_bytes;
    k.row_bytes = (int32_t)col.row_bytes;
    auto fits = [&](size_t v) {
      return aligned(col.ring, v) && aligned(col.rows, v) && col.row_bytes % (int64_t)v == 0 &&
             col.rows_stride_bytes % (int64_t)v == 0;
    };
    k.vec = fits(16) ? 16 : (fits(4) ? 4 : 1);
  }
  a.cursor = reinterpret_cast<unsigned long long*>(q->cursor);
  a.ncols = q->ncols;
  a.capacity = q->capacity;
  return HK_OK;
}

unsigned tiles(int rows) { return (unsigned)(((int64_t)rows + kReplayTile - 1) / kReplayTile); }

}  // namespace

extern "C" {

int hk_replay_push(const hk_replay_desc* q, void* stream) {
  if (const int st = check_desc(q)) return st;
  if (q->batch < 0 || q->batch >= q->capacity) return HK_ERR_SHAPE;
  if (q->batch == 0) return HK_OK;
  ReplayArgs a{};
  if (const int st = fill_args(q, a)) return st;
  a.keep = q->keep;
  a.batch = q->batch;
  return launch_kernel(replay_push_kernel, dim3(tiles(a.batch)), dim3(kReplayThreads), 0, (hipStream_t)stream, a);
}

int hk_replay_sample(const hk_replay_desc* q, int batch_size, uint64_t seed, int64_t* index_out, void* stream) {
  if (const int st = check_desc(q)) return st;
  if (batch_size < 0) return HK_ERR_SHAPE;
  if (batch_size == 0) return HK_OK;
  ReplayArgs a{};
  if (const int st = fill_args(q, a)) return st;
  if (!aligned(index_out, 8)) return HK_ERR_ALIGN;
  a.index_out = index_out;
  a.seed = seed;
  a.batch_size = batch_size;
  return launch_kernel(replay_sample_kernel, dim3(tiles(batch_size)), dim3(kReplayThreads), 0, (hipStream_t)stream, a);
}

}  // extern "C"
