// Stand-alone host program: the union-find core of uz_postproc.hip (unet_zoo_amd/csrc/uz_postproc_core.h, the very text the
// kernels compile) over adversarial planes, sequentially and from 8 threads that share one parent plane, against a flood fill
// written here.  Built by tests/test_postproc.py with the host compiler and -fsanitize=address,undefined and run as a child
// process; it is not loaded into Python and does not touch a GPU.  Exit status: 0 = every plane agrees, 1 = a mismatch or a
// tripped loop bound (this is where an endless find would be caught).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "../unet_zoo_amd/csrc/uz_postproc_core.h"

namespace {

struct Plane {
  std::string name;
  int H, W;
  std::vector<unsigned char> v;
  Plane(const char* n, int h, int w) : name(n), H(h), W(w), v((size_t)h * w, 0) {}
  unsigned char& at(int i, int j) { return v[(size_t)i * W + j]; }
  bool in(int i, int j) const { return i >= 0 && j >= 0 && i < H && j < W && v[(size_t)i * W + j] != 0; }
};

// smallest linear index of every pixel's component (-1 outside the set), by flood fill
std::vector<int> flood(const Plane& p, int conn) {
  std::vector<int> root((size_t)p.H * p.W, -1), stack;
  for (int s = 0; s < p.H * p.W; ++s) {
    if (!p.v[s] || root[s] >= 0) continue;
    root[s] = s;                          // raster order: the first pixel met is the smallest
    stack.push_back(s);
    while (!stack.empty()) {
      const int q = stack.back(), i = q / p.W, j = q % p.W;
      stack.pop_back();
      for (int di = -1; di <= 1; ++di)
        for (int dj = -1; dj <= 1; ++dj) {
          if ((di == 0 && dj == 0) || (conn == 1 && di != 0 && dj != 0)) continue;
          if (!p.in(i + di, j + dj)) continue;
          const int t = (i + di) * p.W + j + dj;
          if (root[t] < 0) root[t] = s, stack.push_back(t);
        }
    }
  }
  return root;
}

// what postproc_init_kernel does: the first pixel of the pixel's run inside its 64-pixel word
void init(const Plane& p, std::vector<int>& parent) {
  const int HW = p.H * p.W;
  for (int w0 = 0; w0 < HW; w0 += 64) {
    unsigned long long in = 0, rs = 0;
    for (int l = 0; l < 64 && w0 + l < HW; ++l) {
      if (p.v[w0 + l]) in |= 1ull << l;
      if ((w0 + l) % p.W == 0) rs |= 1ull << l;
    }
    for (int l = 0; l < 64 && w0 + l < HW; ++l) parent[w0 + l] = p.v[w0 + l] ? w0 + pp_run_start(in, rs, l) : w0 + l;
  }
}

// what postproc_merge_kernel does for the pixels first, first + step, ...
int merge(const Plane& p, int conn, int* parent, int first, int step) {
  const int HW = p.H * p.W, W = p.W;
  int rc = 0;
  for (int q = first; q < HW; q += step) {
    if (!p.v[q]) continue;
    const int i = q / W, j = q % W;
    const unsigned links = pp_links(conn, (q & 63) == 0, p.in(i, j - 1), p.in(i, j + 1), p.in(i - 1, j - 1), p.in(i - 1, j), p.in(i - 1, j + 1));
    if (links & PP_LEFT) rc |= pp_union(parent, q, q - 1, HW);
    if (links & PP_UP) rc |= pp_union(parent, q, q - W, HW);
    if (links & PP_UPLEFT) rc |= pp_union(parent, q, q - W - 1, HW);
    if (links & PP_UPRIGHT) rc |= pp_union(parent, q, q - W + 1, HW);
  }
  return rc;
}

int check(const Plane& p, int conn, int threads) {
  const int HW = p.H * p.W;
  std::vector<int> parent(HW);
  init(p, parent);
  int rc = 0;
  if (threads == 1) {
    rc = merge(p, conn, parent.data(), 0, 1);
  } else {
    std::vector<int> rcs(threads, 0);
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t) pool.emplace_back([&, t] { rcs[t] = merge(p, conn, parent.data(), t, threads); });
    for (auto& th : pool) th.join();
    for (int r : rcs) rc |= r;
  }
  if (rc != 0) {
    std::printf("FAIL %s conn %d threads %d: a loop bound tripped\n", p.name.c_str(), conn, threads);
    return 1;
  }
  const std::vector<int> want = flood(p, conn);
  for (int q = 0; q < HW; ++q) {
    if (!p.v[q]) continue;
    const int got = pp_find(parent.data(), q, HW);
    if (got != want[q]) {
      std::printf("FAIL %s conn %d threads %d: pixel %d has root %d, flood fill says %d\n", p.name.c_str(), conn, threads, q, got, want[q]);
      return 1;
    }
  }
  return 0;
}

std::vector<Plane> planes() {
  std::vector<Plane> out;
  const int H = 33, W = 70;
  out.emplace_back("empty", H, W);
  {
    Plane p("full", H, W);
    for (auto& x : p.v) x = 1;
    out.push_back(p);
  }
  {
    Plane p("corners", H, W);
    p.at(0, 0) = p.at(0, W - 1) = p.at(H - 1, 0) = p.at(H - 1, W - 1) = 1;
    out.push_back(p);
  }
  {
    Plane p("row", 1, 150), q("column", 150, 1);
    for (int k = 0; k < 150; ++k) p.v[k] = q.v[k] = (k % 7 != 3);
    out.push_back(p);
    out.push_back(q);
  }
  {
    Plane p("serpentine", H, W);          // full even rows, joined alternately at the right and the left end
    for (int i = 0; i < H; ++i)
      for (int j = 0; j < W; ++j) p.at(i, j) = i % 2 == 0 || j == ((i / 2) % 2 == 0 ? W - 1 : 0);
    out.push_back(p);
  }
  {
    Plane p("spiral", H, W);
    int t = 0, b = H - 1, l = 0, r = W - 1, i = 0, j = 0;
    // a one-pixel path spiralling inwards with a one-pixel gap between its turns
    while (t <= b && l <= r) {
      for (j = l; j <= r; ++j) p.at(t, j) = 1;
      for (i = t; i <= b; ++i) p.at(i, r) = 1;
      if (b - t >= 2) for (j = r; j >= l + 2; --j) p.at(b, j) = 1;
      if (r - l >= 2) for (i = b; i >= t + 2; --i) p.at(i, l + 2) = 1;
      t += 2, b -= 2, l += 2, r -= 2;
      if (t <= b && l <= r) p.at(t, l) = 1;
    }
    out.push_back(p);
  }
  {
    Plane p("comb_last_row", H, W);       // the roots must travel upwards
    for (int i = 0; i < H; ++i)
      for (int j = 0; j < W; ++j) p.at(i, j) = j % 2 == 0 || i == H - 1;
    out.push_back(p);
  }
  {
    Plane p("comb_last_column", 3, 130);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 130; ++j) p.at(i, j) = i % 2 == 0 || j == 129;
    out.push_back(p);
  }
  {
    Plane p("checkerboard", H, W);
    for (int i = 0; i < H; ++i)
      for (int j = 0; j < W; ++j) p.at(i, j) = (i + j) % 2 == 0;
    out.push_back(p);
  }
  {
    Plane p("diagonal_touch", H, W);
    for (int i = 2; i < 10; ++i)
      for (int j = 3; j < 20; ++j) p.at(i, j) = 1;
    for (int i = 10; i < 20; ++i)
      for (int j = 20; j < 66; ++j) p.at(i, j) = 1;
    out.push_back(p);
  }
  {
    Plane p("noise", 37, 150);
    unsigned s = 12345u;
    for (auto& x : p.v) s = s * 1664525u + 1013904223u, x = (s >> 24) < 150;
    out.push_back(p);
  }
  return out;
}

}  // namespace

int main() {
  int bad = 0, runs = 0;
  for (const Plane& p : planes())
    for (int conn = 1; conn <= 2; ++conn) {
      bad += check(p, conn, 1);
      for (int rep = 0; rep < 4; ++rep) bad += check(p, conn, 8);
      runs += 5;
    }
  // the selection key: larger area first, then the smaller root
  if (!(pp_key(5, 9) > pp_key(4, 0) && pp_key(5, 3) > pp_key(5, 9) && pp_key_area(pp_key(7, 11)) == 7 && pp_key_root(pp_key(7, 11)) == 11 &&
        pp_key(1, 0x7FFFFFFE) > 0ull)) {
    std::printf("FAIL selection key\n");
    ++bad;
  }
  std::printf("%d runs, %d failed\n", runs, bad);
  return bad ? 1 : 0;
}
