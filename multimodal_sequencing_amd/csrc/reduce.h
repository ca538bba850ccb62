// Internal entry points that cross translation units (not part of the C ABI): the deterministic
// reductions of per-workgroup partial rows. Included by the file that defines each and by every
// file that calls it.
#pragma once
#include "common.h"

// ws: [nb][W] partials; ws2: scratch of mmseq_plan::reduce_extra(nb, W) floats.
// columns [0, split) go to outA, [split, W) to outB (either may be NULL).
mmseq_status mmseq_reduce_partials(int nb, int W, int split, const float* ws, float* ws2,
                                   float* outA, float* outB, int accumulate, hipStream_t s);

// three outputs: columns [0, split) to outA, [split, split2) to outB, [split2, W) to outC
mmseq_status mmseq_reduce_partials3(int nb, int W, int split, int split2, const float* ws, float* ws2,
                                    float* outA, float* outB, float* outC, int accumulate,
                                    hipStream_t s);

// LayerNorm-affine gradients (layernorm.hip): dg / db += the column sums of ws [nb][2][cols], which
// has mmseq_plan::reduce_extra(nb, 2 * cols) scratch floats behind it
mmseq_status ln_reduce_partials(int nb, int cols, const float* ws, float* dg, float* db,
                                hipStream_t s);
