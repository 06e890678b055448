// The union-find core of uz_postproc.hip, compiled for the device and for the host alike: find, union, the links a pixel has to
// make for both connectivities, the run start of a pixel inside a 64-pixel word, and the selection key.  The kernels and the
// stand-alone host program tests/postproc_core_main.cpp (sequential and 8 threads on one parent plane, under the sanitizers)
// run this very text; only the two atomic wrappers differ.
//
// parent[x] <= x always, and a parent only ever DECREASES (every write is an atomic min).  A root is a pixel with
// parent[x] == x; the root of a finished component is its smallest linear index.  A reader that sees an old parent of x sees a
// pixel that was united with x before: it is still in x's set and its own chain still ends at the set's root, so a stale
// parent costs steps, never correctness.  That is why relaxed atomics of agent scope suffice although the L2s of the XCDs are
// not coherent with each other: no reader depends on seeing the latest write, and no loop waits for one.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PP_HD __host__ __device__ __forceinline__
#else
#define PP_HD inline
#endif

#define PP_NONE (-1)   // find / union: the loop bound tripped

#if defined(__HIP_DEVICE_COMPILE__)
PP_HD int pp_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
PP_HD int pp_fetch_min(int* p, int v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
PP_HD int pp_clz64(unsigned long long v) { return __clzll((long long)v); }
#else
PP_HD int pp_load(const int* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
PP_HD int pp_fetch_min(int* p, int v) {
  int old = __atomic_load_n(p, __ATOMIC_RELAXED);
  // a retry of the compare-and-swap, never a wait: it fails only because somebody else's write went through
  while (old > v && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
  }
  return old;
}
PP_HD int pp_clz64(unsigned long long v) { return __builtin_clzll(v); }
#endif

// the root of x's chain, or PP_NONE after `bound` steps (a chain is strictly decreasing, so H * W steps is a true bound)
PP_HD int pp_find(const int* parent, int x, int bound) {
  for (int s = 0; s <= bound; ++s) {
    const int p = pp_load(parent + x);
    if (p == x) return x;
    x = p;
  }
  return PP_NONE;
}

// find, then point x at what was found (one atomic min: the chain behind x gets shorter for everybody)
PP_HD int pp_find_compress(int* parent, int x, int bound) {
  const int r = pp_find(parent, x, bound);
  if (r != PP_NONE && r != x) pp_fetch_min(parent + x, r);
  return r;
}

// unite the sets of a and b; 0, or PP_NONE when a bound tripped.  Every failed round replaces (a, b) by two pixels that are
// both smaller than the larger root of the round, so H * W rounds is a true bound here too.
PP_HD int pp_union(int* parent, int a, int b, int bound) {
  for (int s = 0; s <= bound; ++s) {
    a = pp_find_compress(parent, a, bound);
    b = pp_find_compress(parent, b, bound);
    if (a == PP_NONE || b == PP_NONE) return PP_NONE;
    if (a == b) return 0;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = pp_fetch_min(parent + hi, lo);
    if (old == hi) return 0;    // hi was a root and now hangs below lo
    a = old;                    // hi had been given a parent meanwhile: that parent and lo belong together too
    b = lo;
  }
  return PP_NONE;
}

// The pixels of a 64-pixel word (consecutive linear indices) that are in the set: `in`; those that are the first of their
// picture row: `rowstart`.  Returns the lane of the first pixel of lane's run inside the word (lane must be in the set): the
// initial parent, so that a row run is one tree from the start and chains are 64 times shorter.
PP_HD int pp_run_start(unsigned long long in, unsigned long long rowstart, int lane) {
  const unsigned long long starts = in & ~((in << 1) & ~rowstart);
  const unsigned long long upto = starts & (~0ull >> (63 - lane));
  return 63 - pp_clz64(upto);
}

#define PP_LEFT 1
#define PP_UPLEFT 2
#define PP_UP 4
#define PP_UPRIGHT 8
// The links pixel p (in the set) has to make, from which of its neighbours are in the set (outside the picture: false).
// conn 1 = cross, 2 = 3 x 3 square.  `first` = p is the first pixel of its 64-pixel word: a run that goes on from the word
// before has two initial trees there.  (Not `parent[p] == p`: somebody may have moved that parent already.)  The rest of
// the neighbourhood is implied: p and its left neighbour are one run; if the left and the upper-left pixel are in the set,
// the left pixel (or one further left) has tied the two rows together already; in the square an upper-left diagonal is left
// to the left pixel, which has it straight above, and an upper-right one to the right pixel.
PP_HD unsigned pp_links(int conn, bool first, bool l, bool r, bool ul, bool u, bool ur) {
  unsigned m = 0;
  if (l && first) m |= PP_LEFT;
  if (u && !(l && ul)) m |= PP_UP;
  if (conn == 2 && !u) {
    if (ul && !l) m |= PP_UPLEFT;
    if (ur && !r) m |= PP_UPRIGHT;
  }
  return m;
}

// Selection key of a component: larger area first, ties to the smaller root.  One unsigned 64-bit maximum picks the winner,
// whatever the order of arrival.  0 is no component (an area is at least 1).
PP_HD unsigned long long pp_key(int area, int root) {
  return ((unsigned long long)(unsigned)area << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)root);
}
PP_HD int pp_key_area(unsigned long long k) { return (int)(k >> 32); }
PP_HD int pp_key_root(unsigned long long k) { return (int)(0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull)); }
