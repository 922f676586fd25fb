// Stream mode: the launch interface of hg_flow_scan_kernel (hg_flows.hip) for Face A (hg_hsface.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "hg_core.h"

constexpr uint32_t HG_FLOW_ITEM_CLOSE = 1;  // HgFlowItem::flags: the stream's data ends with this write (close / reset / LAST)
// A launch's writes are copied to HBM once when (bytes x workgroups per item) reaches this (measured)
constexpr uint64_t HG_FLOW_HBM_MIN_DEFAULT = 1u << 20;

// One write of a batch.  Its bytes are text[text_off, text_off + len), text_off a multiple of 16, readable up to len
// rounded up to 16.
struct HgFlowItem {
  uint64_t text_off;
  uint32_t len;
  uint32_t flags;
};

struct HgFlowArgs {
  const HgPattern *patterns;  // the database's tables on the device
  const uint32_t *pool;
  uint32_t npatterns;
  const uint8_t *text;         // pinned staging area, or its copy in HBM
  const HgFlowItem *items;     // pinned
  const uint32_t *soff;        // device: offset of each expression's words in a stream's state (header word, then nw state words)
  const uint32_t *state_in;    // pinned: items x swords, the streams' states before the writes
  uint32_t *state_out;         // pinned: ... and after them
  HgHit *out;                  // pinned: reports {pattern << 32 | item, id, position in the write + 1}
  uint32_t cap;                // records `out` holds (more reports: h_flag[0] says how many, the caller repeats with room)
  uint32_t ngroups;            // workgroups per item: ceil(npatterns / HG_FLOW_PPW)
  uint32_t swords;             // words of one stream's state
  uint32_t seq;                // written to h_flag[1] when every workgroup is done
  uint32_t *d_total, *d_done;  // device counters, zero between launches (the last workgroup resets them)
  uint32_t *h_flag;            // pinned: [0] reports of the launch, [1] sequence number
  // start of match (HS_MODE_SOM_HORIZON_*): hg_flow_som_kernel runs the SOM expressions, one lane per (item, expression),
  // before hg_flow_scan_kernel, which leaves them alone.  nsom == 0: not launched.
  const uint32_t *som_list;  // device: the nsom SOM expressions, then per SOM expression the nodes of those before it
  uint32_t nsom;
  uint32_t som_width;        // bytes per carried start: 2, 4 or 8
  int64_t *som_work;         // device: nitems x 2 x (nodes of all SOM expressions) starts (hg_flow_som_kernel has the layout)
  int64_t *from_out;         // pinned, beside `out`: a SOM expression's report's write-relative start
};

// Launches hg_flow_som_kernel (if args.nsom) then hg_flow_scan_kernel over nitems items; 0 or -1.
int hg_flow_launch(const HgFlowArgs &args, uint32_t nitems, hipStream_t stream);
