// The key-padding mask as ag_tile.h's policy, stated once for the two ops that run the core under it: attn_grad.hip (queries X, keys Mem)
// and scene_attn_grad.hip (one source: the chunk's own rows are the keys).  Internal linkage, like ag_tile.h.
#pragma once
#include "ag_tile.h"

namespace {

// pad [contexts of the launch, Lk] or null.  Under the query's lane (ag_fwd, ag_dq) a masked key is a -inf beside the staged tile, 0
// otherwise, ADDED to the score in ag_fwd (s + 0: a row maximum of -0 is stored as +0); under the key's lane (ag_dkv) it is the lane's
// own flag.
struct AgPadMask {
  const unsigned char* pad;
  bool kvalid;
  static constexpr bool REVERSE = false;
  struct KeyTile { float bias[64]; };
  struct QueryTile {};
  __device__ void set_query(int b, int, int Lk) { if (pad) pad += (long)b * Lk; }
  __device__ void set_key(int b, int, int key, int Lk) { kvalid = key < Lk && !(pad && pad[(long)b * Lk + key]); }
  __device__ int key_end(int, int, int Lk) const { return Lk; }
  __device__ int first_query(int) const { return 0; }
  __device__ bool beyond(int, int) const { return false; }
  __device__ int band(int) const { return AG_NO_BAND; }
  __device__ void stage_keys(KeyTile& t, int k0, int Lk, int tid) const {
    if (tid < 64) t.bias[tid] = (k0 + tid < Lk && !(pad && pad[k0 + tid])) ? 0.f : -__builtin_inff();
  }
  __device__ void stage_queries(QueryTile&, int, int) const {}
  __device__ float score(const KeyTile& t, float s, int jj) const { return s + t.bias[jj]; }
  __device__ bool key_visible(const KeyTile& t, int jj) const { return t.bias[jj] == 0.f; }
  __device__ bool query_visible(const QueryTile&, int) const { return kvalid; }
};
// the policy for the contexts of a launch from c0 on
inline AgPadMask ag_pad_mask(const unsigned char* key_pad, int c0, int Lk) { return AgPadMask{key_pad ? key_pad + (long)c0 * Lk : nullptr, false}; }

}  // namespace
