/*
 * gedepth_accum.h — C ABI of the gradient accumulation of libgedepth_hip.so (csrc/accum.hip): the second gradient arena of the fused
 * optimizer (mmrt/optim.py), which sums the gradients of several iterations before one AdamW step.
 *
 * Same conventions as gedepth_hip.h (extern "C", 0 on success, GE_ERR_* of that header for argument errors, device pointers owned by the
 * caller, `stream` a hipStream_t, nothing allocates or synchronises, every check comes before a launch).  Declared here and not in
 * gedepth_hip.h: that header is the versioned training / inference ABI, and it does not change with this.
 */
#ifndef GEDEPTH_ACCUM_H
#define GEDEPTH_ACCUM_H

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ge_grad_accum: one streaming pass over n f32 elements.
 *   first != 0   acc[i] = grad[i].  The old contents of acc are never read (they may be NaN or uninitialised): the first iteration of a
 *                window needs no memset pass.
 *   first == 0   acc[i] = acc[i] + grad[i]: one IEEE f32 add per element (`fp contract(off)`), NaN and inf propagate like any add.
 *   sumsq        null, or one f64: sumsq[0] += sum of (double)a * a over the values a just stored, ge_sumsq's convention (the caller zeroes
 *                it; one atomic add per workgroup, so the order of the partial sums is not fixed).  With null no reduction code runs.
 * The last iteration of a window so yields the accumulated gradient and its squared norm in one pass.
 * n == 0 returns 0 without a launch.  GE_ERR_BAD_ARG: a null acc or grad, n < 0, acc or grad not 16-byte aligned, sumsq not 8-byte
 * aligned, acc == grad.
 */
int ge_grad_accum(float* acc, const float* grad, long n, int first, double* sumsq, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GEDEPTH_ACCUM_H */
