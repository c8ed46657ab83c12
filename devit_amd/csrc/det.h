// Deterministic mode (internal; det.hip): the process-wide switch, the caller-owned workspace the fixed-order reductions keep their partial
// sums in, and the kernels that finish them.  With the mode on, a site whose addresses receive several partial sums writes every partial with a
// plain store to its own place in the workspace -- part[slab s][...], s = the slice / strip / workgroup INDEX -- and a fold launch behind it computes
//     out <- fp32(out + fold),   fold = (((p_0 + p_1) + p_2) + ... + p_{S-1})   in fp32, left to right,
// one thread per output element.  No workgroup waits for another; the order is the index order whatever the arrival order was.
#pragma once
#include "devit_common.h"

namespace devit_det {

bool on();   // devit_set_deterministic / DEVIT_DETERMINISTIC=1 (read once)

// The registered workspace of the current device as floats, at least `need_bytes` of it: DEVIT_ERR_ARG with a message otherwise (never a fall-back
// to the atomics).  ws == NULL: the check alone.
int workspace(const char* who, size_t need_bytes, float** ws);

// out[b * out_bs + r * ldc + c] += fold over s < S of part[(b * S + s) * slab + r * cols + c],   b < batch, r < rows, c < cols
int fold(const float* part, int S, size_t slab, int rows, int cols, float* out, long long ldc, int batch, long long out_bs, hipStream_t s);

}  // namespace devit_det
