// The ONE dropout mask definition of the library (include/devit_hip.h, "Dropout"): counter-based, never stored; a backward regenerates
// what its forward used.  Philox4x32-10 (Salmon et al., SC'11), key = the two halves of the per-forward seed, counter =
// (group lo, group hi, site, block) with group = e >> 2 for the element's logical index e = row * pitch + col (pitch % 4 == 0): one call
// serves four consecutive columns of a row, element e takes output word e & 3 and is KEPT iff word >= thr.
#pragma once
#include "devit_common.h"

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

enum { DROP_SITE_POS = 0, DROP_SITE_ATTN = 1, DROP_SITE_PROJ = 2, DROP_SITE_HIDDEN = 3, DROP_SITE_FC2 = 4, DROP_SITES = 5 };

struct DropKey {       // what a kernel needs of one (seed, site, block, p)
  unsigned k0, k1;     // seed & 0xffffffff, seed >> 32
  unsigned site, block;
  unsigned thr;        // keep iff word >= thr;  thr = min(floor(p * 2^32), 2^32 - 1), from the host
  float s;             // 1 / (1 - p): kept values are multiplied by it in fp32
};
inline DropKey drop_key(unsigned long long seed, int site, int block, unsigned thr, float s) {
  return DropKey{(unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), (unsigned)site, (unsigned)block, thr, s};
}

__device__ __forceinline__ u32x4 philox4x32_10(u32x4 c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    c = (u32x4){hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0};
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}
// the four words of elements e0 .. e0 + 3 (e0 % 4 == 0)
__device__ __forceinline__ u32x4 drop_words(const DropKey& d, unsigned long long e0) {
  const unsigned long long g = e0 >> 2;
  return philox4x32_10((u32x4){(unsigned)g, (unsigned)(g >> 32), d.site, d.block}, d.k0, d.k1);
}
