// speckle_math.h — the rule of the speckle filter (include/odometry_hip.h, odo_speckle_create), host + device
// like stereo_depth_math.h: the kernels of speckle_kernels.hip, the host object (speckle_api.hip.h, the bounds it validates) and the
// g++ harness of tests/speckle_math_harness.cpp compile these same lines. The connection predicate, the survival test and the
// parameter check are each written once, here, with a sequential reference labelling over dense planes. Integers only: a component
// is a class of a transitive closure and its size a count, so nothing depends on the order of evaluation.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ODO_SP_HD __host__ __device__ __forceinline__
#else
#define ODO_SP_HD static inline
#endif

namespace odo {

constexpr int kSpMaxSize = 8192;                    // rows, cols: a linear pixel index fits int32
constexpr int kSpMaxDiff = 65535;                   // max_diff
constexpr int kSpMaxMinSize = 1 << 30;              // min_size
constexpr int kSpNoLabel = -1;                      // parent of a pixel whose key is 0
constexpr int kSpStatWords = 8;                     // pixels, components, removed_components, removed_pixels, largest, 0, 0, 0
static_assert((long long)kSpMaxSize * kSpMaxSize < (1LL << 31), "a linear pixel index and a component's size fit int32");

// The bounds odo_speckle_create validates, in the order of the specification. 0: fine; otherwise the number of the bound that fails
// (1 size, 2 max_diff, 3 min_size).
ODO_SP_HD int sp_check_params(int rows, int cols, int max_diff, int min_size) {
  if (rows < 1 || cols < 1 || rows > kSpMaxSize || cols > kSpMaxSize) return 1;
  if (max_diff < 0 || max_diff > kSpMaxDiff) return 2;
  if (min_size < 1 || min_size > kSpMaxMinSize) return 3;
  return 0;
}

// Two 4-neighbours with keys a and b are connected iff both keys are non-zero and differ by at most max_diff.
ODO_SP_HD bool sp_connected(int a, int b, int max_diff) {
  const int d = a - b;
  return a != 0 && b != 0 && (d < 0 ? -d : d) <= max_diff;
}

// A non-zero pixel survives iff its component has at least min_size pixels.
ODO_SP_HD bool sp_survives(int size, int min_size) { return size >= min_size; }

// ---- the reference labelling over dense rows x cols planes (the kernels label tiles in LDS and unite them across the seams instead) --
// The root of pixel i: parent[] only ever points to a smaller index of the same component, so the walk ends.
ODO_SP_HD int sp_ref_find(const int32_t* parent, int i) {
  while (parent[i] != i) i = parent[i];
  return i;
}

// parent[i] = the smallest linear index of pixel i's component (kSpNoLabel where key[i] == 0); size[i] = that component's pixel count
// at its root, 0 elsewhere. Sequential: every pixel is united with its left and its upper neighbour, the larger root under the smaller.
ODO_SP_HD void sp_ref_label(const uint16_t* key, int rows, int cols, int max_diff, int32_t* parent, int32_t* size) {
  for (int y = 0; y < rows; y++)
    for (int x = 0; x < cols; x++) {
      const int i = y * cols + x;
      size[i] = 0;
      parent[i] = key[i] ? i : kSpNoLabel;
      if (!key[i]) continue;
      const int nb[2] = {x > 0 ? i - 1 : -1, y > 0 ? i - cols : -1};
      for (int k = 0; k < 2; k++) {
        if (nb[k] < 0 || !sp_connected(key[i], key[nb[k]], max_diff)) continue;
        const int a = sp_ref_find(parent, i), b = sp_ref_find(parent, nb[k]);
        if (a < b) parent[b] = a;
        else parent[a] = b;
      }
    }
  const int n = rows * cols;
  for (int i = 0; i < n; i++)
    if (parent[i] >= 0) {
      parent[i] = sp_ref_find(parent, i);   // (parent[i] <= i: every earlier pixel already points at its root)
      size[parent[i]] += 1;
    }
}

// The filter's end for dense planes: every non-surviving pixel is zeroed in a (and in b unless it is NULL); out[kSpStatWords] gets the
// counters. parent and size as sp_ref_label leaves them.
ODO_SP_HD void sp_ref_apply(const int32_t* parent, const int32_t* size, int rows, int cols, int min_size, uint16_t* a, uint16_t* b,
                            int64_t* out) {
  for (int k = 0; k < kSpStatWords; k++) out[k] = 0;
  const int n = rows * cols;
  for (int i = 0; i < n; i++) {
    if (parent[i] < 0) continue;
    const int sz = size[parent[i]];
    const bool keep = sp_survives(sz, min_size);
    out[0] += 1;
    if (parent[i] == i) {
      out[1] += 1;
      out[2] += !keep;
      if (sz > out[4]) out[4] = sz;
    }
    if (!keep) {
      out[3] += 1;
      a[i] = 0;
      if (b) b[i] = 0;
    }
  }
}

}  // namespace odo
