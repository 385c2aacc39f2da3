/*
 * atr_stem_full.h — C ABI of the whole-map conv stem in libtrack2d_hip.so (csrc/stem_full_hip.hip): CNN_maze's two convolutions
 * on the 'Full' ids' single-channel frames of side S = 81 (Maze maps) or 82 (Block / Empty maps), float32:
 *
 *     z1 = relu(conv(1 -> 16, k3, s2, p1)(x))     S x S   -> 41 x 41   (never leaves the kernel)
 *     y  = relu(conv(16 -> 32, k3, s2, p1)(z1))   41 x 41 -> 21 x 21
 *
 * Both sides give 41 and 21; they differ only in the last tap of z1's row / column 40 (S = 81: padding, S = 82: cell 81).
 * Frame m starts at x + m * x_stride floats (rows contiguous, x_stride >= S * S: one agent's planes of the env's [N, 2, S, S]
 * tensor are read in place with x_stride = 2 * S * S). y is [M, 32 * 21 * 21] in (c, h, w) order. Weights are the nn.Conv2d
 * layouts: w1 [16, 1, 3, 3], b1 [16], w2 [32, 16, 3, 3], b2 [32]. All pointers are device pointers to float32; `stream` is a
 * hipStream_t. Every function but the workspace query returns 0, -1 (bad arguments; nothing was launched) or -2 (launch failed).
 * The first call of any of them sets the backward kernel's dynamic-LDS limit: make it outside a stream capture.
 */
#ifndef ATR_STEM_FULL_H
#define ATR_STEM_FULL_H

#ifdef __cplusplus
extern "C" {
#endif

/* y = stem(x) for M frames. M == 0 returns 0 without a launch; S other than 81 / 82 returns -1. */
int atr_stem_full_forward(const float *x, long long x_stride, int S, const float *w1, const float *b1, const float *w2,
                          const float *b2, float *y, long long M, void *stream);

/* Floats of workspace atr_stem_full_backward needs for M frames: one 4800-float partial record (dw2 4608, db2 32, dw1 144,
 * db1 16) per workgroup of its grid, which is min(3 M, 2 x compute units) — three row bands per frame. */
long long atr_stem_full_workspace_floats(long long M);

/* The four parameter gradients of sum(y * dy) over the M frames; the frames get none. y is the forward's output (its ReLU
 * mask), dy [M, 32 * 21 * 21]; z1 is recomputed from x. dw1 [144], db1 [16], dw2 [4608], db2 [32] are overwritten. The grid,
 * the frames each workgroup takes and the order of the one reduction pass over the records depend on M alone: two calls on the
 * same inputs give the same bits. M == 0 returns 0 without a launch (outputs untouched). */
int atr_stem_full_backward(const float *x, long long x_stride, int S, const float *y, const float *dy, const float *w1,
                           const float *b1, const float *w2, float *dw1, float *db1, float *dw2, float *db2, float *workspace,
                           long long M, void *stream);

#ifdef __cplusplus
}
#endif

#endif
