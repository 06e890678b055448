// Host-side scaffold of the descriptor passes (augment, patch, surface, confusion, postproc, tile and the composed losses):
// the address-range refusals, the workspace layout, the grid cap and the item table of the composed losses.  Plain host
// C++, included by uz_common.h after UZ_REQUIRE and UZ_NUM_CU_HW; no device code.
#pragma once
#include <math.h>
#include <stdint.h>

// ---- address ranges ----------------------------------------------------------------------------------------------------
// [lo, hi) of a tensor; a null pointer (an optional tensor that was not passed) or no bytes is the empty range {0, 0},
// which overlaps nothing.
struct UzRange {
  uintptr_t lo, hi;
};
static inline UzRange uz_range(const void* p, long long bytes) {
  if (p == nullptr || bytes <= 0) return {0, 0};
  return {(uintptr_t)p, (uintptr_t)p + (uintptr_t)bytes};
}
static inline bool uz_overlap(const UzRange& x, const UzRange& y) { return x.lo < y.hi && y.lo < x.hi; }
// What a call writes against everything else it touches: does an output overlap an input or another output?  With
// n_in = 0 the pairwise test over one list.
static inline bool uz_any_overlap(const UzRange* outs, int n_out, const UzRange* ins, int n_in) {
  for (int a = 0; a < n_out; ++a) {
    for (int b = 0; b < n_in; ++b)
      if (uz_overlap(outs[a], ins[b])) return true;
    for (int b = a + 1; b < n_out; ++b)
      if (uz_overlap(outs[a], outs[b])) return true;
  }
  return false;
}

// ---- workspace layout --------------------------------------------------------------------------------------------------
static inline long long uz_align16(long long b) { return (b + 15) / 16 * 16; }
// n buffers one after the other, each on a 16-byte boundary: off[e] = where buffer e starts; returns the bytes of all
static inline long long uz_carve(const long long* sizes, int n, long long* off) {
  long long at = 0;
  for (int e = 0; e < n; ++e) {
    off[e] = at;
    at += uz_align16(sizes[e]);
  }
  return at;
}

// ---- grids -------------------------------------------------------------------------------------------------------------
// per_cu workgroups per CU of the hardware is what can be resident at once; more units than that are walked
static inline int uz_grid_cap(long long units, int per_cu) {
  const long long cap = (long long)per_cu * UZ_NUM_CU_HW;
  return (int)(units < cap ? units : cap);
}

// ---- the item table of the composed losses (uz_boundary_loss, uz_lovasz_loss, uz_cldice_loss, uz_hardpixel_loss) ---------
// Checks every item, appends its logits to ins[] and its dlogits (where given) to outs[], notes whether any map takes a
// gradient, and fills the kernel-argument table tab[UZ_CLASS_MAX_ITEMS], padded with item 0.
static inline int uz_map_items(const char* who, const uz_map_item* items, int n_items, long long map_bytes, UzRange* ins, int* n_in,
                               UzRange* outs, int* n_out, bool* any_grad, uz_map_item* tab) {
  *any_grad = false;
  for (int i = 0; i < n_items; ++i) {
    const uz_map_item& it = items[i];
    UZ_REQUIRE(it.logits != nullptr, "%s: item %d has null logits", who, i);
    UZ_REQUIRE((((uintptr_t)it.logits | (uintptr_t)it.dlogits) & 3) == 0, "%s: tensors must be 4-byte aligned", who);
    UZ_REQUIRE(it.weight >= 0.f && it.weight < INFINITY, "%s: item %d has a negative weight", who, i);
    ins[(*n_in)++] = uz_range(it.logits, map_bytes);
    if (it.dlogits != nullptr) {
      outs[(*n_out)++] = uz_range(it.dlogits, map_bytes);
      *any_grad = true;
    }
    tab[i] = it;
  }
  for (int i = n_items; i < UZ_CLASS_MAX_ITEMS; ++i) tab[i] = tab[0];
  return UZ_OK;
}
