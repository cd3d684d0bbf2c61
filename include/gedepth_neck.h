/*
 * gedepth_neck.h — C ABI of the HAHI neck's level-token kernels of libgedepth_hip.so (csrc/nhwc.hip): the (B, N, C) token matrix whose N rows
 * are the concatenated levels of a feature pyramid, N = sum N_l, written, read and summed level by level where it lives.
 *
 * Same conventions as gedepth_hip.h (extern "C", 0 on success, GE_ERR_* of that header for argument errors, device pointers owned by
 * the caller, `stream` a hipStream_t, dtype GE_F32 / GE_BF16, nothing allocates or synchronises).  Declared here and not in gedepth_hip.h:
 * that header is the versioned training / inference ABI, and it does not change with these.
 *
 * A level table is `level_starts`: n_levels + 1 row indices on the HOST, read during the call and handed to the kernels by value:
 * level_starts[0] == 0, non-decreasing, level_starts[n_levels] == N, 1 <= n_levels <= GE_NECK_MAX_LEVELS.  Level l owns rows
 * [level_starts[l], level_starts[l + 1]) of every image; an empty level is allowed.
 *
 * All kernels need C % (16 / element size) == 0, at most 256 16-byte vectors per row and 16-byte aligned pointers (GE_ERR_UNSUPPORTED
 * otherwise).  Every check comes before a launch.
 */
#ifndef GEDEPTH_NECK_H
#define GEDEPTH_NECK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GE_NECK_MAX_LEVELS 8

/*
 * ge_bn_act_nhwc_fwd_rows / ge_bn_act_nhwc_bwd_rows: ge_bn_act_nhwc_fwd / _bwd (gedepth_hip.h) with a free image stride on `y` (forward)
 * and on `dy` (backward).  The dense operands are (rows, C) with rows = B * rows_per_image; row r of them is row
 * (r / rows_per_image) * image_stride + r % rows_per_image of the strided one (image_stride in rows, >= rows_per_image).  Only that
 * address differs: the row-to-workgroup mapping and the order of every sum are those of the dense entry points, so statistics, running
 * statistics, output and gradients carry the same bits.  Workspace: ge_nhwc_workspace(C, 2) bytes.
 * GE_ERR_BAD_ARG: what the dense entry points reject, rows % rows_per_image != 0 or image_stride < rows_per_image.
 */
int ge_bn_act_nhwc_fwd_rows(const void* x, const float* gamma, const float* beta, void* y, long rows_per_image, long image_stride,
                            float* save_mean, float* save_rstd, float* running_mean, float* running_var, void* workspace, long rows, int C,
                            float eps, float momentum, float slope, int dtype, void* stream);
/* the activation decision is recomputed from x with `beta` (the forward's shift), as ge_bn_act_nhwc_bwd does when it is given */
int ge_bn_act_nhwc_bwd_rows(const void* dy, long rows_per_image, long image_stride, const void* x, const float* gamma, const float* beta,
                            const float* save_mean, const float* save_rstd, void* dx, float* dgamma, float* dbeta, void* workspace, long rows,
                            int C, float slope, int dtype, void* stream);

/*
 * ge_add_rows_levels: out[b, n, :] = x[b, n, :] + (pos[n, :] + emb[level(n), :]).  x, out (B, N, C) dense; pos (N, C) f32; emb
 * (n_levels, C) f32.  The inner sum is one f32 add and the outer one is rounded once into the storage type: the bits of ge_add_rows on
 * rows that were formed as pos + emb in f32.
 */
int ge_add_rows_levels(const void* x, const float* pos, const float* emb, void* out, int B, long N, int C, const long* level_starts,
                       int n_levels, int dtype, void* stream);

/*
 * ge_level_colsum: out[l, c] = sum over the images and the rows of level l of x[b, n, c].  x (B, N, C) dense, out (n_levels, C) f32; an
 * empty level gives zeros.  One read of x: f32 per thread, one f32 partial per (workgroup, level, channel), then the f64 fold of
 * ge_colsum.  Workspace: ge_nhwc_workspace(C, n_levels) bytes.
 */
int ge_level_colsum(const void* x, int B, long N, int C, const long* level_starts, int n_levels, float* out, void* workspace, int dtype,
                    void* stream);

/*
 * ge_token_grad_sum: out = a0 [+ a1] [+ a2] [+ parts], summed in f32 in that order and rounded once.  a0 .. a2 and out are (B, N, C) dense;
 * a1, a2 may be null, and so may a0 when there are parts.  Parts (n_parts == 0: none; then level_starts is not read): one per level,
 * element (b, n, c) of level l's rows is read in place at parts[l] + (b * N_l + n) * pitch[l] + col[l] + c, i.e. out of a dense
 * (B * N_l, pitch[l]) matrix of the same storage type.  parts, pitch, col: n_parts entries on the HOST, read during the call.
 * GE_ERR_BAD_ARG: no source at all, a null part of a non-empty level, col[l] < 0 or col[l] + C > pitch[l].  GE_ERR_UNSUPPORTED as above,
 * and a pitch or column offset that is not a whole number of 16-byte vectors.
 */
int ge_token_grad_sum(const void* a0, const void* a1, const void* a2, const void* const* parts, const long* pitch, const long* col,
                      const long* level_starts, int n_parts, void* out, int B, long N, int C, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GEDEPTH_NECK_H */
