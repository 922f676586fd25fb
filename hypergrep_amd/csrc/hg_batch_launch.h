// Batched block scan: the launch interface of hg_block_batch_kernel (hg_batch.hip) for Face A (hg_hsface.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "hg_batch.h"

constexpr uint32_t HG_BATCH_MAX_WGS = 1024;  // workgroups of one launch at most (groups x shards): four per CU, two of them resident

struct HgBatchArgs {
  const HgPattern *patterns;  // the database's tables on the device
  const uint32_t *pool;
  uint32_t npatterns;
  uint32_t ppw, ngroups;       // expressions per workgroup, groups (hg_block_small_grouping, hg_engine.h)
  uint32_t nshards;            // workgroups per group; shard s takes items s, s + nshards, ...
  const uint8_t *text;         // pinned staging area, or its copy in HBM
  const HgBatchItem *items;    // pinned, or its copy in HBM (with the text)
  uint32_t nitems;
  HgHit *out;                  // pinned: reports {item of the launch, id, to | HG_HIT_SINGLE_BIT}
  uint32_t cap;                // records `out` holds (more reports: h_flag[0] says how many, the caller repeats with room)
  uint32_t seq;                // written to h_flag[1] when every workgroup is done
  uint32_t *d_total, *d_done;  // device counters, zero between launches (the last workgroup resets them)
  uint32_t *h_flag;            // pinned: [0] reports of the launch, [1] sequence number
};

// Launches hg_block_batch_kernel over args.ngroups x args.nshards workgroups; 0 or -1.
int hg_batch_launch(const HgBatchArgs &args, hipStream_t stream);
