/*
 * cloudsc2_hip.h - C ABI of the MI355X-native CLOUDSC2 column-physics engine (libcloudsc2_hip.so).
 *
 * Each entry point replaces ONE GT4Py stencil object of the reference, i.e. the callable that
 * `compile_stencil(name, externals)` returns and that the components invoke with keyword field
 * arguments (`self.cloudsc2(in_ap=..., ..., dt=..., origin=(0,0,0), domain=(nx,1,nz+1), ...)`).
 * The reference call sites are cited per function below (paths relative to
 * /root/reference/src/cloudsc2_gt4py/physics/).
 *
 * Conventions shared by every entry point
 *   - plain C types only; no torch / HIP types in the signatures (`stream` is a hipStream_t
 *     passed as void*, NULL = the legacy default stream);
 *   - all field pointers are DEVICE pointers (HBM) owned by the caller; the library never
 *     allocates, frees or copies fields;
 *   - field layout is [level][column]: element (column c, level k) of a field lives at
 *     ptr[k * lev_stride + c], 0 <= c < nx, 0 <= k <= nz (every field has nz+1 levels, as every
 *     reference storage has, nonlinear/microphysics.py:168-169; the padding level nz of a
 *     full-level field is never written and, for `lu`, must be 0, nonlinear/_stencils/cloudsc2.py:212);
 *   - `eta` is a device vector of nz+1 values (`in_eta`, gtscript.Field[K]);
 *   - pointer-array arguments (`in`, `out`) are HOST arrays of device pointers in the order of
 *     the enum documented with the function (= the order of the gtscript signature);
 *   - the boolean externals LPHYLIN / LDRAIN1D / LEVAPLS2 / LREGCL / IGNORE_SUPSAT select a kernel
 *     instantiation, the numeric externals travel by value in `Cloudsc2Params`;
 *   - return value: 0 on success, <0 on error (CLOUDSC2_E_*); `cloudsc2_last_error()` returns a
 *     thread-local message.  Kernels are launched asynchronously on `stream`;
 *   - threading: the library is written for ONE host thread per process and device (the one-process-per-GPU
 *     model of the drivers).  Error text is thread-local, the kernel-name diagnostic process-wide (an atomic pointer to a literal); the per-device facts the
 *     launchers cache (CU count, the >64 KiB LDS opt-in of the ring kernels) are relaxed atomics whose only race
 *     is a repeated, idempotent query, so a second thread launching on the same device is safe.  Device ordinals
 *     >= 64 are refused (CLOUDSC2_E_UNSUPPORTED);
 *   - inputs and outputs of one call must not overlap (no in-place calls): the kernels stream level by level
 *     and cloudsc2_ad re-reads its inputs in its second sweep.  The Python stencil objects check this when
 *     called with validate_args=True.
 */
#ifndef CLOUDSC2_HIP_H
#define CLOUDSC2_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Stays 4 with the cloudsc2_saturation_tl_* / _ad_*, cloudsc2_tl_step_* / _ad_step_* and cloudsc2_*_enss_* entries: they are purely additive
 * (no existing prototype, enum or struct changed), so a caller built against the earlier version 4 header runs unchanged. */
#define CLOUDSC2_ABI_VERSION 4

#define CLOUDSC2_OK 0
#define CLOUDSC2_E_ARG (-1)      /* bad argument (null pointer, nx/nz/stride out of range)      */
#define CLOUDSC2_E_UNSUPPORTED (-2) /* no kernel for this call: ICALL != 0, or a FUSED build extension (cloudsc2_nl_fused_*,
                                       _nl_taylor*, _tl_incremented_*) on fields of 4 GiB or more ((nz+1) * lev_stride *
                                       sizeof(element) must be < 2^32 there).  cloudsc2_nl / _tl / _ad themselves take
                                       fields of any size: beyond 4 GiB they run their 64-bit-offset instantiation */
#define CLOUDSC2_E_LAUNCH (-3)   /* HIP reported an error at launch                              */
#define CLOUDSC2_E_NODEVICE (-4) /* no HIP device visible                                        */

/* Numeric + boolean externals (names = /root/reference/src/cloudsc2_gt4py/iox.py:25-209 and the
 * literals of nonlinear/microphysics.py:68-78, common/saturation.py:51, common/increment.py:47-49).
 * Mirrored field-for-field by `Cloudsc2Params` in gt4py_dwarf_p_cloudsc2_tl_ad_amd/params.py. */
typedef struct Cloudsc2Params {
    double R2ES, R3IES, R3LES, R4IES, R4LES, R5IES, R5LES;
    double R5ALSCP, R5ALVCP, RALSDCP, RALVDCP;
    double RTICE, RTWAT, RTWAT_RTICE_R, RTICECU, RTWAT_RTICECU_R, RVTMP2;
    double RCPD, RD, RETV, RG, RLMLT, RLSTT, RLVTT, RTT;
    double RCLCRIT, RKCONV, RLMIN, RPECONS, RLPTRC;
    double ZEPS1, ZEPS2, ZQMAX, ZSCAL, QMAX;
    int32_t LPHYLIN, LDRAIN1D, LEVAPLS2, LREGCL, ICALL, KFLAG, IGNORE_SUPSAT, NLEV;
    /* Build extension, NOT a reference external (default 0 = reproduce the reference literally).
     * 1: cloudsc2_ad uses the freezing tests of the NL/TL stencils (post-adjustment t < RTT at
     * adjoint/_stencils/cloudsc2.py:427,:577; the forward test of :343 at :729), which makes AD the
     * exact transpose of TL also in columns where the saturation adjustment crosses RTT
     * (SURVEY.md Appendix B Q4/Q5). */
    int32_t AD_TRAJ_FIX;
} Cloudsc2Params;

int32_t cloudsc2_abi_version(void);
int32_t cloudsc2_params_sizeof(void);
const char* cloudsc2_last_error(void);
/* diagnostics: name of the kernel the process's last successful entry-point call enqueued, whichever thread made it
 * (torch.autograd runs a backward pass on a thread of its own), e.g.
 * "cs2::nl_ring_kernel" (LDS-ring load path) or "cs2::nl_kernel" (register prefetch); "" before the first launch */
const char* cloudsc2_last_kernel(void);
/* number of HIP devices visible to the library's runtime (0 if none / runtime unusable) */
int32_t cloudsc2_device_count(void);

/* ---- cloudsc2_nl : nonlinear/_stencils/cloudsc2.py:24-399, called at nonlinear/microphysics.py:134-172 */
enum { /* order of `in` */
    NL_IN_AP, NL_IN_APH, NL_IN_LU, NL_IN_LUDE, NL_IN_MFD, NL_IN_MFU, NL_IN_Q, NL_IN_QI, NL_IN_QL,
    NL_IN_QSAT, NL_IN_SUPSAT, NL_IN_T, NL_IN_TND_CML_Q, NL_IN_TND_CML_QI, NL_IN_TND_CML_QL,
    NL_IN_TND_CML_T, NL_NUM_IN
};
enum { /* order of `out` */
    NL_OUT_CLC, NL_OUT_COVPTOT, NL_OUT_FHPSL, NL_OUT_FHPSN, NL_OUT_FPLSL, NL_OUT_FPLSN,
    NL_OUT_TND_Q, NL_OUT_TND_QI, NL_OUT_TND_QL, NL_OUT_TND_T, NL_NUM_OUT
};
int32_t cloudsc2_nl_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                        const double* const* in, const double* eta, double* const* out, double dt,
                        void* stream);
int32_t cloudsc2_nl_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                        const float* const* in, const float* eta, float* const* out, double dt,
                        void* stream);

/* ---- cloudsc2_nl, fused variants (BUILD EXTENSIONS - the reference has no such stencil).
 * Exactly one of `qsat_out` / `in_i` is non-NULL; results are those of the separate stencil calls.
 *   qsat_out != NULL : `saturation` (LPHYLIN form, common/_stencils/saturation.py:30-35,42) is evaluated inside the
 *                      NL kernel from in[NL_IN_AP], in[NL_IN_T]; in[NL_IN_QSAT] is not read (may be NULL) and the
 *                      result is written to qsat_out: the driver's timed region (run_nonlinear.py:117-118) in ONE launch.
 *   in_i != NULL     : every input is read as in[f] + pf * in_i[f] (perturbed_state, perturbed_state.py:75-91): the
 *                      Taylor test's perturbed NL runs (tangent_linear/validation.py:166-176) without the perturbed copy. */
int32_t cloudsc2_nl_fused_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                              const double* const* in, const double* const* in_i, double pf, double* qsat_out,
                              const double* eta, double* const* out, double dt, void* stream);
int32_t cloudsc2_nl_fused_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                              const float* const* in, const float* const* in_i, double pf, float* qsat_out,
                              const float* eta, float* const* out, double dt, void* stream);

/* ---- perturbed NL run + Taylor-test reduction (BUILD EXTENSION, SURVEY.md 8f rank 1, third item).
 * Replaces, per step size, perturbed_state + cloudsc2_nl + the ten field differences and sums of
 * TaylorTest.run / get_field_norm (tangent_linear/validation.py:166-176, :239-249): NL is evaluated on in + pf * in_i,
 * nothing is stored, and workgroup b writes  partials[b * NL_NUM_OUT + f] = sum over its columns and all levels of
 * (NL(in + pf in_i) - ref_out)[f]  in double precision (f in NL_OUT_* order; ref_out = the unperturbed NL outputs,
 * read-only).  `partials` is a DEVICE array of cloudsc2_nl_taylor_blocks(nx) * NL_NUM_OUT doubles; the caller adds
 * the blocks (fixed order: deterministic). */
int32_t cloudsc2_nl_taylor_blocks(int32_t nx);
int32_t cloudsc2_nl_taylor_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                               const double* const* in, const double* const* in_i, double pf, const double* eta,
                               const double* const* ref_out, double* partials, double dt, void* stream);
int32_t cloudsc2_nl_taylor_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                               const float* const* in, const float* const* in_i, double pf, const float* eta,
                               const float* const* ref_out, double* partials, double dt, void* stream);

/* ---- the Taylor test's perturbed runs for SEVERAL step sizes per launch (BUILD EXTENSION).
 * Replaces the whole loop of TaylorTest.run (tangent_linear/validation.py:162-176: perturbed_state, cloudsc2_nl, get_norm
 * per step size): a lane loads the 16 state + 16 increment + 10 reference words of a level once and evaluates the level
 * for up to 5 step sizes on them (internally ceil(nf / 5) launches), so the perturbed runs are bound by arithmetic instead
 * of re-streaming 42 words per level, column and step size.  `in_i` may be NULL: the increments are then formed in the
 * kernel as T(inc_f) * in (state_increment fused in, state_increment.py:61-80; p->IGNORE_SUPSAT zeroes the supsat
 * increment), otherwise inc_f is ignored.  `pf`: HOST array of the nf step sizes; `partials`: DEVICE
 * array of cloudsc2_nl_taylor_blocks(nx) * nf * NL_NUM_OUT doubles, partials[(b * nf + j) * NL_NUM_OUT + f] = sum over
 * workgroup b's columns and all levels of (NL(in + pf[j] in_i) - ref_out)[f]; the caller adds the blocks. */
int32_t cloudsc2_nl_taylor_multi_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                     const double* const* in, const double* const* in_i, double inc_f, int32_t nf,
                                     const double* pf, const double* eta, const double* const* ref_out, double* partials,
                                     double dt, void* stream);
int32_t cloudsc2_nl_taylor_multi_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                     const float* const* in, const float* const* in_i, double inc_f, int32_t nf,
                                     const double* pf, const float* eta, const float* const* ref_out, double* partials,
                                     double dt, void* stream);

/* ---- validation-norm reductions (BUILD EXTENSIONS; the reference reduces on the host with NumPy).
 * field_sums : per field f < nfields (<= 16), sum over nlev levels and nx columns of a[f] - b[f] (b == NULL: of a[f]);
 *              the difference is formed in the field type, accumulated in double - TaylorTest.get_field_norm's
 *              np.sum(field_nl_p - field_nl) and np.sum(field_tl) (tangent_linear/validation.py:250-261).  Workgroup w
 *              writes partials[w * nfields + f]; `partials` holds cloudsc2_field_sums_blocks(nx, nlev) * nfields doubles.
 * column_dots: per column c, the sum over pairs p < npairs (<= 16) and nlev levels of a[p][k][c] * b[p][k][c] in double -
 *              SymmetryTest.get_norm1 / get_norm2 (adjoint/validation.py:167-215) - delivered as level-chunk partials:
 *              out[j * nx + c] (+)= the sum over chunk j's levels, j < cloudsc2_column_dots_chunks(nlev); the caller adds
 *              the chunks.  `accumulate` != 0 adds to what `out` holds (for more than 16 pairs: a second call). */
int32_t cloudsc2_field_sums_blocks(int32_t nx, int32_t nlev);
int32_t cloudsc2_column_dots_chunks(int32_t nlev);
int32_t cloudsc2_field_sums_f64(int32_t nx, int32_t nlev, int64_t lev_stride, int32_t nfields, const double* const* a,
                                const double* const* b, double* partials, void* stream);
int32_t cloudsc2_field_sums_f32(int32_t nx, int32_t nlev, int64_t lev_stride, int32_t nfields, const float* const* a,
                                const float* const* b, double* partials, void* stream);
int32_t cloudsc2_column_dots_f64(int32_t nx, int32_t nlev, int64_t lev_stride, int32_t npairs, const double* const* a,
                                 const double* const* b, double* out, int32_t accumulate, void* stream);
int32_t cloudsc2_column_dots_f32(int32_t nx, int32_t nlev, int64_t lev_stride, int32_t npairs, const float* const* a,
                                 const float* const* b, double* out, int32_t accumulate, void* stream);

/* ---- saturation : common/_stencils/saturation.py:23-42, called at common/saturation.py:67-76
 * (domain nx x 1 x nz: level nz of out_qsat is not written) */
int32_t cloudsc2_saturation_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                const double* ap, const double* t, double* qsat, void* stream);
int32_t cloudsc2_saturation_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                const float* ap, const float* t, float* qsat, void* stream);

/* ---- tangent-linear and adjoint of `saturation` (BUILD EXTENSIONS - the reference has no such stencil: its harnesses
 * perturb qsat independently).  With, per point of the nx x nz domain of cloudsc2_saturation_* (level nz is never touched),
 *     alfa = min(1, ((max(TI, min(RTWAT, t)) - TI) RI)^2),  el / ei = R2ES exp(R3xES (t - RTT) / (t - R4xES)),
 *     ew = alfa el + (1 - alfa) ei,  qs = min(ew / ap, QMAX),  qsat = qs / (1 - RETV qs)
 * ((TI, RI) = (RTICE, RTWAT_RTICE_R), or (RTICECU, RTWAT_RTICECU_R) when LPHYLIN == 0 and KFLAG == 1), the derivative takes
 * every min / max on the branch the value took, with the value's own comparison; a clamped branch has derivative 0:
 *     alfa' = 2 (t - TI) RI^2 for TI < t < RTWAT, else 0
 *     ew_t  = alfa' (el - ei) + alfa el R3LES (RTT - R4LES) / (t - R4LES)^2 + (1 - alfa) ei R3IES (RTT - R4IES) / (t - R4IES)^2
 *     clipped at QMAX: qs_t = qs_ap = 0;  otherwise qs_t = ew_t / ap, qs_ap = -ew / ap^2
 *     g_t = qs_t / (1 - RETV qs)^2,  g_ap = qs_ap / (1 - RETV qs)^2
 *   TL:  qsat_i = g_t t_i + g_ap ap_i.   ap_i or t_i may be NULL (a zero perturbation; at least one is not);
 *        qsat may be NULL (the value is not written; when written it equals cloudsc2_saturation_*'s bit for bit).
 *   AD:  t_adj (+)= g_t qsat_adj,  ap_adj (+)= g_ap qsat_adj.   ap_adj or t_adj may be NULL (that adjoint is not wanted; at
 *        least one is not); accumulate != 0 adds to what they hold - e.g. the t / ap adjoints cloudsc2_ad_masked_* has just
 *        written, which completes the adjoint of saturation + cloudsc2_nl.
 * All three forms (LPHYLIN; KFLAG == 1 / other).  Argument errors are settled on the host before any launch, with the
 * argument's name in cloudsc2_last_error(); nx == 0 is a successful no-op.
 * Words moved per point: TL 2 + (present perturbations) + 1 + (1 if qsat); AD 3 + (wanted adjoints), twice those when
 * accumulating (counted on the expectation that the word loaded in place of an absent field is served from the cache;
 * no counter was read). */
int32_t cloudsc2_saturation_tl_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride, const double* ap,
                                   const double* t, const double* ap_i, const double* t_i, double* qsat, double* qsat_i,
                                   void* stream);
int32_t cloudsc2_saturation_tl_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride, const float* ap,
                                   const float* t, const float* ap_i, const float* t_i, float* qsat, float* qsat_i,
                                   void* stream);
int32_t cloudsc2_saturation_ad_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride, const double* ap,
                                   const double* t, const double* qsat_adj, double* ap_adj, double* t_adj,
                                   int32_t accumulate, void* stream);
int32_t cloudsc2_saturation_ad_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride, const float* ap,
                                   const float* t, const float* qsat_adj, float* ap_adj, float* t_adj,
                                   int32_t accumulate, void* stream);

/* ---- state_increment : common/_stencils/state_increment.py:22-80, called at common/increment.py:93-132
 * ---- perturbed_state : common/_stencils/perturbed_state.py:22-91, called at common/increment.py:219-261
 * Field order of the 16-entry arrays (same for in / in_i / out): */
enum {
    INC_APH, INC_AP, INC_Q, INC_QSAT, INC_T, INC_QL, INC_QI, INC_LUDE, INC_LU, INC_MFU, INC_MFD,
    INC_TND_CML_T, INC_TND_CML_Q, INC_TND_CML_QL, INC_TND_CML_QI, INC_SUPSAT, INC_NUM
};
int32_t cloudsc2_state_increment_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                     const double* const* in, double* const* out_i, double f, void* stream);
int32_t cloudsc2_state_increment_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                     const float* const* in, float* const* out_i, double f, void* stream);
int32_t cloudsc2_perturbed_state_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                     const double* const* in, const double* const* in_i,
                                     double* const* out, double f, void* stream);
int32_t cloudsc2_perturbed_state_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                     const float* const* in, const float* const* in_i,
                                     float* const* out, double f, void* stream);

/* ---- cloudsc2_tl : tangent_linear/_stencils/cloudsc2.py:23-774, called at tangent_linear/microphysics.py:162-242
 * `in` / `in_i`: the 16 NL inputs and their perturbations, NL_IN_* order;
 * `out` / `out_i`: the 10 NL outputs and their perturbations, NL_OUT_* order. */
int32_t cloudsc2_tl_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                        const double* const* in, const double* const* in_i, const double* eta,
                        double* const* out, double* const* out_i, double dt, void* stream);
int32_t cloudsc2_tl_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                        const float* const* in, const float* const* in_i, const float* eta,
                        float* const* out, float* const* out_i, double dt, void* stream);

/* ---- cloudsc2_tl with state_increment fused in (BUILD EXTENSION).  The harnesses call state_increment and cloudsc2_tl back
 * to back on the same state (tangent_linear/validation.py:159-164, adjoint/validation.py:138-143); here the perturbation
 * fields are not read but formed in the kernel as in_i[f] = T(f) * in[f] (state_increment.py:61-80; with
 * p->IGNORE_SUPSAT the supsat perturbation is 0, :77-80): 16 input streams instead of 32 and no increment launch.  The
 * increments are the very products the increment kernel would store; the outputs equal those of the two separate calls up
 * to the compiler's fma contraction of the shared level function (ulps). */
int32_t cloudsc2_tl_incremented_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                    const double* const* in, double f, const double* eta, double* const* out,
                                    double* const* out_i, double dt, void* stream);
int32_t cloudsc2_tl_incremented_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                    const float* const* in, double f, const float* eta, float* const* out,
                                    float* const* out_i, double dt, void* stream);

/* ---- cloudsc2_ad : adjoint/_stencils/cloudsc2.py:24-996, called at adjoint/microphysics.py:159-238
 * `in`     : the 16 NL inputs (trajectory), NL_IN_* order;
 * `in_adj` : adjoint forcing = perturbations of the 10 NL outputs, NL_OUT_* order
 *            (in_clc_i, in_covptot_i, in_fhpsl_i, in_fhpsn_i, in_fplsl_i, in_fplsn_i,
 *             in_tnd_q_i, in_tnd_qi_i, in_tnd_ql_i, in_tnd_t_i); NOT modified (the reference
 *            zeroes them in place, adjoint/_stencils/cloudsc2.py:481-484 ...; nothing reads them
 *            afterwards);
 * `out`    : the 10 NL outputs recomputed along the trajectory, NL_OUT_* order;
 * `out_adj`: adjoint of the 16 inputs, NL_IN_* order (out_ap_i ... out_tnd_cml_t_i). */
int32_t cloudsc2_ad_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                        const double* const* in, const double* const* in_adj, const double* eta,
                        double* const* out, double* const* out_adj, double dt, void* stream);
int32_t cloudsc2_ad_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                        const float* const* in, const float* const* in_adj, const float* eta,
                        float* const* out, float* const* out_adj, double dt, void* stream);

/* ---- cloudsc2_ad WITHOUT its forward sweep (BUILD EXTENSION).  The symmetry test calls cloudsc2_tl and then cloudsc2_ad on
 * the same state (adjoint/validation.py:135-151).  The kernel behind cloudsc2_ad_* recomputes the NL trajectory in a first
 * sweep only to obtain, per level, the rain / snow fluxes entering it - and those are the NL outputs out_fplsl / out_fplsn
 * the TL call has just written.  Here they are READ (`traj_fplsl`, `traj_fplsn`: (nz+1)-level fields as cloudsc2_nl /
 * cloudsc2_tl write them) and the forward sweep is skipped: 44 words per level and column instead of 70.  Nothing but
 * `out_adj` is written (the recomputed NL outputs of cloudsc2_ad_* are not produced: they are the TL call's).  With fluxes
 * that come from cloudsc2_ad_*'s own `out` the adjoints are bit-identical to that call's; with a TL call's they agree to
 * rounding (the two kernels contract the same formulas differently) only if AD_TRAJ_FIX = 1 or no column's saturation
 * adjustment crosses RTT: with AD_TRAJ_FIX = 0 (quirk Q4) cloudsc2_ad's forward sweep freezes on the pre-adjustment
 * temperature and cloudsc2_tl on the post-adjustment one, so in such columns the TL fluxes are not cloudsc2_ad's and the
 * result is neither cloudsc2_ad's adjoint nor the TL transpose.  Driver switches only: LEVAPLS2 / LDRAIN1D are
 * refused (CLOUDSC2_E_UNSUPPORTED), as are fields of 4 GiB and more. */
int32_t cloudsc2_ad_from_trajectory_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                        const double* const* in, const double* const* in_adj, const double* eta,
                                        const double* traj_fplsl, const double* traj_fplsn, double* const* out_adj, double dt,
                                        void* stream);
int32_t cloudsc2_ad_from_trajectory_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                        const float* const* in, const float* const* in_adj, const float* eta,
                                        const float* traj_fplsl, const float* traj_fplsn, float* const* out_adj, double dt,
                                        void* stream);

/* ---- cloudsc2_tl / cloudsc2_ad with ABSENT fields (BUILD EXTENSIONS): the linearisation as a derivative rule.
 * The reference calls its TL and AD stencils with all 52 fields (tangent_linear/microphysics.py:162-242,
 * adjoint/microphysics.py:159-238).  A Jacobian-vector or vector-Jacobian product taken by an automatic-differentiation
 * framework has perturbations / forcing on a few fields only and wants a few results only; every field it does not have
 * or does not want is HBM traffic of the dense calls.  Here such fields are NULL entries:
 *   in       16 entries, NL_IN_* order, all required (the trajectory);
 *   in_i     (TL) 16 entries, NL_IN_* order;  NULL entry = that perturbation is zero everywhere;
 *   in_adj   (AD) 10 entries, NL_OUT_* order; NULL entry = that forcing is zero everywhere;
 *   out      (TL) NULL as a whole (the NL outputs are not written), or 10 non-NULL entries, NL_OUT_* order;
 *   out_i    (TL) 10 entries, NL_OUT_* order, and
 *   out_adj  (AD) 16 entries, NL_IN_* order:  NULL entry = that field is not written; at least one entry is non-NULL;
 *   zero_line  caller-owned DEVICE memory of at least 512 zero bytes, 16-byte aligned, read-only: what the kernels read in
 *            place of an absent input (every wave reads the same line, which therefore stays in cache; the library still
 *            never allocates).  May be NULL when no entry of in_i / in_adj is NULL;
 *   traj_fplsl / traj_fplsn  (AD) required: out_fplsl / out_fplsn of a cloudsc2_nl / cloudsc2_tl call on the same state, as
 *            for cloudsc2_ad_from_trajectory_*, whose restrictions the AD entry keeps: LEVAPLS2 / LDRAIN1D are refused
 *            (CLOUDSC2_E_UNSUPPORTED).
 * Both entries keep 32-bit byte offsets: fields of 4 GiB and more are refused (CLOUDSC2_E_UNSUPPORTED) - use the dense
 * stencils there.  The TL entry takes every combination of externals cloudsc2_tl takes.  Argument errors are settled on
 * the host before any launch; nx == 0 is a successful no-op.
 * A field that is written equals what the dense call writes for the same inputs with zero fields in place of the absent
 * ones: for AD bit for bit (the arithmetic of cloudsc2_ad_from_trajectory_*), for TL to rounding (the compiler contracts
 * the shared level function per kernel).
 * Words moved per level and column: TL 16 + (present in_i) + (10 if out) + (present out_i) against 52 of cloudsc2_tl;
 * AD 16 + 2 + (present in_adj) + (present out_adj) against 44 of cloudsc2_ad_from_trajectory and 70 of cloudsc2_ad - e.g.
 * forcing on the four tendencies and adjoints of t, q, ql, qi: 26. */
int32_t cloudsc2_tl_masked_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                               const double* const* in, const double* const* in_i, const double* zero_line,
                               const double* eta, double* const* out, double* const* out_i, double dt, void* stream);
int32_t cloudsc2_tl_masked_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                               const float* const* in, const float* const* in_i, const float* zero_line,
                               const float* eta, float* const* out, float* const* out_i, double dt, void* stream);
int32_t cloudsc2_ad_masked_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                               const double* const* in, const double* const* in_adj, const double* zero_line,
                               const double* eta, const double* traj_fplsl, const double* traj_fplsn,
                               double* const* out_adj, double dt, void* stream);
int32_t cloudsc2_ad_masked_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                               const float* const* in, const float* const* in_adj, const float* zero_line,
                               const float* eta, const float* traj_fplsl, const float* traj_fplsn,
                               float* const* out_adj, double dt, void* stream);

/* ---- the derivative of the whole step, saturation + cloudsc2_nl, in one launch (BUILD EXTENSIONS - no reference stencil).
 * cloudsc2_nl_fused_* with qsat_out is the step; these are its tangent-linear and its adjoint: the masked entries above with
 * the derivative of `saturation` (the rule documented with cloudsc2_saturation_tl_* / _ad_*) fused in, so the path
 * t, ap -> qsat -> cloudsc2 is part of the result.  Arguments are those of cloudsc2_tl_masked_* / cloudsc2_ad_masked_*, and
 * so are the size (fields below 4 GiB), zero-line and evaporation-switch rules (the AD entry refuses LEVAPLS2 / LDRAIN1D),
 * with these differences:
 *   in[NL_IN_QSAT]       is not read and may be NULL: the kernel forms qsat from in[NL_IN_AP] and in[NL_IN_T], bit for bit
 *                        what cloudsc2_nl_fused_* / cloudsc2_saturation_* compute;
 *   LPHYLIN              only this form of saturation is available fused, as for cloudsc2_nl_fused_*: anything else is
 *                        CLOUDSC2_E_UNSUPPORTED (compose cloudsc2_saturation_tl_* / _ad_* with the masked entries);
 *   in_i[NL_IN_QSAT]     (TL) must be NULL (CLOUDSC2_E_ARG): the perturbation the level sees is g_t t_i + g_ap ap_i, formed
 *                        from that level's words.  This one NULL entry needs no zero line;
 *   out_adj[NL_IN_QSAT]  (AD) must be NULL (CLOUDSC2_E_ARG): the level's qsat adjoint is not stored but folded, as
 *                        g_t qsat_adj into out_adj[NL_IN_T] and as g_ap qsat_adj into out_adj[NL_IN_AP].  Only those two:
 *                        out_adj[NL_IN_TND_CML_T] stays dt times the t adjoint of cloudsc2 itself.
 * cloudsc2_last_kernel() reports "cs2::tl_step_kernel" / "cs2::ad_step_kernel".
 * Words moved per level and column: TL 15 + (present in_i) + (10 if out) + (present out_i) - two words less than
 * cloudsc2_saturation_tl + cloudsc2_tl_masked, and one launch less; AD 15 + 2 + (present in_adj) + (present out_adj), where
 * the composition moves 16 + 2 + ... + 1 (the qsat adjoint) in cloudsc2_ad_masked and then reads 3 fields and
 * read-modify-writes 2 in cloudsc2_saturation_ad - e.g. forcing on the four tendencies and adjoints of t, q, ql, qi: 25
 * words in one launch against about 34 in two. */
int32_t cloudsc2_tl_step_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                             const double* const* in, const double* const* in_i, const double* zero_line,
                             const double* eta, double* const* out, double* const* out_i, double dt, void* stream);
int32_t cloudsc2_tl_step_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                             const float* const* in, const float* const* in_i, const float* zero_line,
                             const float* eta, float* const* out, float* const* out_i, double dt, void* stream);
int32_t cloudsc2_ad_step_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                             const double* const* in, const double* const* in_adj, const double* zero_line,
                             const double* eta, const double* traj_fplsl, const double* traj_fplsn,
                             double* const* out_adj, double dt, void* stream);
int32_t cloudsc2_ad_step_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                             const float* const* in, const float* const* in_adj, const float* zero_line,
                             const float* eta, const float* traj_fplsl, const float* traj_fplsn,
                             float* const* out_adj, double dt, void* stream);

/* ---- cloudsc2_tl_masked / cloudsc2_tl_step for SEVERAL DIRECTIONS on one trajectory (BUILD EXTENSIONS): a Jacobian block,
 * an ensemble of perturbations pushed through one linearisation.  Arguments are those of cloudsc2_tl_masked_* (multi) and
 * of cloudsc2_tl_step_* (multi_step), and so are their rules (NULL entries, zero line, LPHYLIN for the step, fields below
 * 4 GiB PER DIRECTION), plus:
 *   ndir            number of directions, 1 .. CLOUDSC2_TL_MAX_DIRS (CLOUDSC2_E_ARG otherwise);
 *   in_dir_stride   in ELEMENTS: in_i[f] points at direction 0 of a batched field, direction d of every present
 *                   perturbation starts d * in_dir_stride elements later;
 *   out_dir_stride  in ELEMENTS: the same for every wanted out_i[f].
 * Both strides must be at least (nz+1) * lev_stride (CLOUDSC2_E_ARG): the directions of a field do not overlap.  A field is
 * present or absent for all directions alike.  `out` (the NL outputs) is not batched: it is written once.
 * One launch reads the trajectory once: the kernel keeps the five perturbation words of each direction's carried state in
 * LDS (5 * ndir * 256 elements per workgroup beside the level table) and loops over the directions inside each level.  Every
 * direction of every written field equals what the single-direction entry writes for that direction alone.
 * cloudsc2_last_kernel() reports "cs2::tl_dirs_kernel" / "cs2::tl_dirs_step_kernel".
 * Words moved per level and column: 16 (step: 15) + ndir * ((present in_i) + (present out_i)) + (10 if out). */
#define CLOUDSC2_TL_MAX_DIRS 8
int32_t cloudsc2_tl_multi_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                              const double* const* in, const double* const* in_i, const double* zero_line,
                              const double* eta, double* const* out, double* const* out_i, double dt, void* stream,
                              int32_t ndir, int64_t in_dir_stride, int64_t out_dir_stride);
int32_t cloudsc2_tl_multi_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                              const float* const* in, const float* const* in_i, const float* zero_line,
                              const float* eta, float* const* out, float* const* out_i, double dt, void* stream,
                              int32_t ndir, int64_t in_dir_stride, int64_t out_dir_stride);
int32_t cloudsc2_tl_multi_step_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                   const double* const* in, const double* const* in_i, const double* zero_line,
                                   const double* eta, double* const* out, double* const* out_i, double dt, void* stream,
                                   int32_t ndir, int64_t in_dir_stride, int64_t out_dir_stride);
int32_t cloudsc2_tl_multi_step_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                   const float* const* in, const float* const* in_i, const float* zero_line,
                                   const float* eta, float* const* out, float* const* out_i, double dt, void* stream,
                                   int32_t ndir, int64_t in_dir_stride, int64_t out_dir_stride);

/* ---- cloudsc2_ad_masked / cloudsc2_ad_step for SEVERAL DIRECTIONS on one trajectory (BUILD EXTENSIONS): a block of rows
 * of the Jacobian, several cost functionals or observation sensitivities on one trajectory.  Arguments are those of
 * cloudsc2_ad_masked_* (multi) and of cloudsc2_ad_step_* (multi_step), and so are their rules, all settled on the host
 * before any launch (NULL entries, zero line, at least one wanted adjoint, LEVAPLS2 / LDRAIN1D refused with
 * CLOUDSC2_E_UNSUPPORTED, LPHYLIN and out_adj[NL_IN_QSAT] == NULL for the step, fields below 4 GiB PER DIRECTION;
 * nx == 0 is a successful no-op), plus:
 *   ndir            number of directions, 1 .. CLOUDSC2_AD_MAX_DIRS (CLOUDSC2_E_ARG otherwise);
 *   in_dir_stride   in ELEMENTS: in_adj[f] points at direction 0 of a batched field, direction d of every present forcing
 *                   starts d * in_dir_stride elements later;
 *   out_dir_stride  in ELEMENTS: the same for every wanted out_adj[f].
 * Both strides must be at least (nz+1) * lev_stride (CLOUDSC2_E_ARG): the directions of a field do not overlap.  A field is
 * present or absent for all directions alike.  `traj_fplsl` / `traj_fplsn` (the trajectory) are not batched.
 * One launch reads the trajectory once and recomputes each level's nonlinear state (all its exponentials; for the step,
 * saturation and its derivative too) once: only the backward statements run per direction, in a loop inside each level.
 * LDS per workgroup: the level table, 2 * (nz+1) elements; in fp32 the 34 * 256 parked trajectory elements of the single
 * entries; and the six words of each direction's backward carry, 6 * ndir * 256 elements (ndir = 8, nz = 137: about 98 KB
 * in fp64, 83 KB in fp32).  A call whose demand exceeds 160 KB is refused (CLOUDSC2_E_UNSUPPORTED).
 * Every direction of every written field equals what the single-direction entry writes for that direction alone (the same
 * ad_forward / ad_backward on the same words; to rounding, since the compiler contracts them per kernel).
 * cloudsc2_last_kernel() reports "cs2::ad_dirs_kernel" / "cs2::ad_dirs_step_kernel".
 * Words moved per level and column: 16 (step: 15) + 2 + ndir * ((present in_adj) + (present out_adj)) - e.g. forcing on the
 * four tendencies and adjoints of t, q, ql, qi with the step entry: 17 + 8 ndir against 25 ndir of ndir single launches. */
#define CLOUDSC2_AD_MAX_DIRS 8
int32_t cloudsc2_ad_multi_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                              const double* const* in, const double* const* in_adj, const double* zero_line,
                              const double* eta, const double* traj_fplsl, const double* traj_fplsn,
                              double* const* out_adj, double dt, void* stream,
                              int32_t ndir, int64_t in_dir_stride, int64_t out_dir_stride);
int32_t cloudsc2_ad_multi_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                              const float* const* in, const float* const* in_adj, const float* zero_line,
                              const float* eta, const float* traj_fplsl, const float* traj_fplsn,
                              float* const* out_adj, double dt, void* stream,
                              int32_t ndir, int64_t in_dir_stride, int64_t out_dir_stride);
int32_t cloudsc2_ad_multi_step_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                   const double* const* in, const double* const* in_adj, const double* zero_line,
                                   const double* eta, const double* traj_fplsl, const double* traj_fplsn,
                                   double* const* out_adj, double dt, void* stream,
                                   int32_t ndir, int64_t in_dir_stride, int64_t out_dir_stride);
int32_t cloudsc2_ad_multi_step_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                   const float* const* in, const float* const* in_adj, const float* zero_line,
                                   const float* eta, const float* traj_fplsl, const float* traj_fplsn,
                                   float* const* out_adj, double dt, void* stream,
                                   int32_t ndir, int64_t in_dir_stride, int64_t out_dir_stride);

/* ---- TRAJECTORY ADJOINTS WITH THE EVAPORATION BLOCK (BUILD EXTENSIONS): cloudsc2_ad_masked_*, cloudsc2_ad_step_*,
 * cloudsc2_ad_multi_* and cloudsc2_ad_multi_step_* for LEVAPLS2 / LDRAIN1D, which those entries refuse.
 *       entry                          arguments of                   kernel
 *       cloudsc2_ad_evap_*             cloudsc2_ad_masked_*           cs2::ad_cover_kernel
 *       cloudsc2_ad_evap_step_*        cloudsc2_ad_step_*             cs2::ad_cover_step_kernel
 *       cloudsc2_ad_evap_multi_*       cloudsc2_ad_multi_*            cs2::ad_cover_dirs_kernel
 *       cloudsc2_ad_evap_multi_step_*  cloudsc2_ad_multi_step_*       cs2::ad_cover_dirs_step_kernel
 * plus two arguments - before `stream` in the single entries, behind the direction arguments in the multi entries:
 *   cover        caller-owned DEVICE field of nz+1 levels at the call's lev_stride (the library still never allocates), not
 *                batched over directions.  It must not overlap any other field of the call.  Level nz is never touched.
 *                NULL is CLOUDSC2_E_ARG.
 *   cover_ready  0: the launch fills `cover`, then reads it.  Non-zero: `cover` already holds what such a launch left for the
 *                same state, trajectory fluxes, eta, dt and parameters; it is then read-only.  (The second and later chunks
 *                of more than CLOUDSC2_AD_MAX_DIRS cotangents; repeated backward passes on one forward.)
 * Why: with the evaporation block the precipitation cover ENTERING a level is loop-carried trajectory besides the two
 * fluxes, and no NL output holds it (out_covptot is 0 both where the block did not run and where everything evaporated).
 * Each launch therefore runs two sweeps, one lane per column: sweep 1 (levels 0 .. nz-1; skipped with cover_ready) takes the
 * fluxes entering each level from traj_fplsl / traj_fplsn, recomputes the level and stores the cover entering it to
 * cover[level]; sweep 2 is the masked / step / multi-direction adjoint sweep with the evaporation block, reading cover[level]
 * with the level's words.  in_adj[NL_OUT_COVPTOT] is a forcing like the others; out_adj[NL_IN_APH] at level nz also
 * receives the accumulated adjoint of the surface pressure.  The adjoints equal those of cloudsc2_ad given the same
 * forcing, AD_TRAJ_FIX and a trajectory from cloudsc2_nl, to rounding (each kernel contracts the level functions itself).
 * Everything the masked, step and multi entries check is checked here in the same way; a call with NEITHER LEVAPLS2 nor
 * LDRAIN1D is CLOUDSC2_E_UNSUPPORTED (the message names the entry to use instead); nx == 0 is a successful no-op.
 * LDS of the multi entries: the level table; six carry words per direction (6 * ndir * 256 elements: two pairs of the
 * backward carry are kept as their sums, which is exact); parked trajectory words, 34 * 256 elements in fp32 and 30 * 256
 * in fp64 (there the level's trajectory would not fit the registers across the direction loop).  ndir = 8, nz = 137: about
 * 158 KB in fp64, 83 KB in fp32; beyond 160 KB the call is refused (fp64: ndir = 8 beyond nz = 255).  The
 * ensemble forms of the two single entries are declared at the end of this file ("ENSEMBLES WITH THE EVAPORATION BLOCK").
 * Words moved per level and column: sweep 1 reads 16 (step: 15) + 2 and writes 1; sweep 2 moves 16 (15) + 2 + 1 + ndir *
 * ((present in_adj) + (wanted out_adj)).  Forcing on the four tendencies, adjoints of t, q, ql, qi, one direction:
 * 19 + 19 + 8 = 46 against 70 of cloudsc2_ad; eight directions: 38 + 64 = 102 against 560.  With cover_ready sweep 1's 19
 * drop out. */
int32_t cloudsc2_ad_evap_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                             const double* const* in, const double* const* in_adj, const double* zero_line,
                             const double* eta, const double* traj_fplsl, const double* traj_fplsn,
                             double* const* out_adj, double dt, double* cover, int32_t cover_ready, void* stream);
int32_t cloudsc2_ad_evap_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                             const float* const* in, const float* const* in_adj, const float* zero_line,
                             const float* eta, const float* traj_fplsl, const float* traj_fplsn,
                             float* const* out_adj, double dt, float* cover, int32_t cover_ready, void* stream);
int32_t cloudsc2_ad_evap_step_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                  const double* const* in, const double* const* in_adj, const double* zero_line,
                                  const double* eta, const double* traj_fplsl, const double* traj_fplsn,
                                  double* const* out_adj, double dt, double* cover, int32_t cover_ready, void* stream);
int32_t cloudsc2_ad_evap_step_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                  const float* const* in, const float* const* in_adj, const float* zero_line,
                                  const float* eta, const float* traj_fplsl, const float* traj_fplsn,
                                  float* const* out_adj, double dt, float* cover, int32_t cover_ready, void* stream);
int32_t cloudsc2_ad_evap_multi_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                   const double* const* in, const double* const* in_adj, const double* zero_line,
                                   const double* eta, const double* traj_fplsl, const double* traj_fplsn,
                                   double* const* out_adj, double dt, void* stream,
                                   int32_t ndir, int64_t in_dir_stride, int64_t out_dir_stride,
                                   double* cover, int32_t cover_ready);
int32_t cloudsc2_ad_evap_multi_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                   const float* const* in, const float* const* in_adj, const float* zero_line,
                                   const float* eta, const float* traj_fplsl, const float* traj_fplsn,
                                   float* const* out_adj, double dt, void* stream,
                                   int32_t ndir, int64_t in_dir_stride, int64_t out_dir_stride,
                                   float* cover, int32_t cover_ready);
int32_t cloudsc2_ad_evap_multi_step_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                        const double* const* in, const double* const* in_adj, const double* zero_line,
                                        const double* eta, const double* traj_fplsl, const double* traj_fplsn,
                                        double* const* out_adj, double dt, void* stream,
                                        int32_t ndir, int64_t in_dir_stride, int64_t out_dir_stride,
                                        double* cover, int32_t cover_ready);
int32_t cloudsc2_ad_evap_multi_step_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                        const float* const* in, const float* const* in_adj, const float* zero_line,
                                        const float* eta, const float* traj_fplsl, const float* traj_fplsn,
                                        float* const* out_adj, double dt, void* stream,
                                        int32_t ndir, int64_t in_dir_stride, int64_t out_dir_stride,
                                        float* cover, int32_t cover_ready);

/* ---- ENSEMBLES: the NL step, the masked TL / AD and the step TL / AD for `nmem` MEMBERS in one launch (BUILD EXTENSIONS):
 * an ensemble of model states, per-member gradients, an ML batch.  Unlike the multi-direction entries above EVERYTHING a
 * call has is batched - state, perturbations or forcing, trajectory fluxes, every output, qsat_out - and every member is a
 * complete, independent call.  Arguments are those of the single entry named in the table, followed by:
 *   nmem            number of members, >= 1 (CLOUDSC2_E_ARG otherwise);
 *   member_stride   in ELEMENTS, ONE value for every field of the call: each non-NULL field pointer points at member 0
 *                   and member m of it starts m * member_stride elements later.  At least (nz+1) * lev_stride
 *                   (CLOUDSC2_E_ARG): the members of a field do not overlap.
 *       ensemble entry              single entry                 kernel reported by cloudsc2_last_kernel
 *       cloudsc2_nl_ens_*           cloudsc2_nl_*                cs2::nl_ens_kernel
 *       cloudsc2_nl_fused_ens_*     cloudsc2_nl_fused_*          cs2::nl_ens_kernel<saturation>
 *       cloudsc2_tl_ens_*           cloudsc2_tl_masked_*         cs2::tl_ens_kernel
 *       cloudsc2_tl_step_ens_*      cloudsc2_tl_step_*           cs2::tl_ens_step_kernel
 *       cloudsc2_ad_ens_*           cloudsc2_ad_masked_*         cs2::ad_ens_kernel
 *       cloudsc2_ad_step_ens_*      cloudsc2_ad_step_*           cs2::ad_ens_step_kernel
 * The rules of the single entry hold, all settled on the host before any launch (ICALL, dt > 0, NLEV, NULL entries and the
 * zero line, LEVAPLS2 / LDRAIN1D refused by the adjoints, LPHYLIN for the step and the fused entries; nx == 0 is a
 * successful no-op).  `eta`, `dt`, the switches and the zero line are shared by all members; a field is present or absent
 * for all members alike, and an absent input is read from the zero line by every member.  cloudsc2_nl_fused_ens_* is the
 * saturation-fused form only: qsat_out is required, in_i must be NULL and pf is ignored.
 * Sizes: ONE MEMBER of a field stays below 4 GiB, (nz+1) * lev_stride * sizeof(element) < 2^32 (CLOUDSC2_E_UNSUPPORTED
 * otherwise; the lanes' byte offsets are 32-bit); the ensemble as a whole may be larger - the member's base is added to the
 * field pointers as a 64-bit scalar.  nmem * ceil(nx / 256) workgroups must fit a one-dimensional grid, 2^31 - 1
 * (CLOUDSC2_E_UNSUPPORTED).  Always the register-path kernels (no LDS ring).
 * Every member of every written field equals what the single entry writes for that member alone (the same level functions
 * on the same words).  Elements between the members (member_stride beyond a member's extent) are not touched. */
int32_t cloudsc2_nl_ens_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                            const double* const* in, const double* eta, double* const* out, double dt, void* stream,
                            int32_t nmem, int64_t member_stride);
int32_t cloudsc2_nl_ens_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                            const float* const* in, const float* eta, float* const* out, double dt, void* stream,
                            int32_t nmem, int64_t member_stride);
int32_t cloudsc2_nl_fused_ens_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                  const double* const* in, const double* const* in_i, double pf, double* qsat_out,
                                  const double* eta, double* const* out, double dt, void* stream,
                                  int32_t nmem, int64_t member_stride);
int32_t cloudsc2_nl_fused_ens_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                  const float* const* in, const float* const* in_i, double pf, float* qsat_out,
                                  const float* eta, float* const* out, double dt, void* stream,
                                  int32_t nmem, int64_t member_stride);
int32_t cloudsc2_tl_ens_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                            const double* const* in, const double* const* in_i, const double* zero_line,
                            const double* eta, double* const* out, double* const* out_i, double dt, void* stream,
                            int32_t nmem, int64_t member_stride);
int32_t cloudsc2_tl_ens_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                            const float* const* in, const float* const* in_i, const float* zero_line,
                            const float* eta, float* const* out, float* const* out_i, double dt, void* stream,
                            int32_t nmem, int64_t member_stride);
int32_t cloudsc2_tl_step_ens_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                 const double* const* in, const double* const* in_i, const double* zero_line,
                                 const double* eta, double* const* out, double* const* out_i, double dt, void* stream,
                                 int32_t nmem, int64_t member_stride);
int32_t cloudsc2_tl_step_ens_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                 const float* const* in, const float* const* in_i, const float* zero_line,
                                 const float* eta, float* const* out, float* const* out_i, double dt, void* stream,
                                 int32_t nmem, int64_t member_stride);
int32_t cloudsc2_ad_ens_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                            const double* const* in, const double* const* in_adj, const double* zero_line,
                            const double* eta, const double* traj_fplsl, const double* traj_fplsn,
                            double* const* out_adj, double dt, void* stream, int32_t nmem, int64_t member_stride);
int32_t cloudsc2_ad_ens_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                            const float* const* in, const float* const* in_adj, const float* zero_line,
                            const float* eta, const float* traj_fplsl, const float* traj_fplsn,
                            float* const* out_adj, double dt, void* stream, int32_t nmem, int64_t member_stride);
int32_t cloudsc2_ad_step_ens_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                 const double* const* in, const double* const* in_adj, const double* zero_line,
                                 const double* eta, const double* traj_fplsl, const double* traj_fplsn,
                                 double* const* out_adj, double dt, void* stream, int32_t nmem, int64_t member_stride);
int32_t cloudsc2_ad_step_ens_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                 const float* const* in, const float* const* in_adj, const float* zero_line,
                                 const float* eta, const float* traj_fplsl, const float* traj_fplsn,
                                 float* const* out_adj, double dt, void* stream, int32_t nmem, int64_t member_stride);

/* ---- ENSEMBLES THAT SHARE PART OF THEIR STATE (BUILD EXTENSIONS): the six ensemble entries above for members that differ in
 * a few state fields (t, q, ql, qi of an ensemble of analyses) and share the rest (pressures, convective inputs, supsat, the
 * tnd_cml_*), and whose `eta` may differ per member.  Nothing is copied: a shared field is ONE field, read by every member.
 * Arguments are those of the ensemble entry named in the table, followed by:
 *   shared_mask        bit i (i = NL_IN_*, 0 .. 15; the step and the fused entries use the same indices) set: in[i] is ONE
 *                      field, the call's pointer, read by every member; clear: in[i] is batched, member m lies
 *                      m * member_stride elements behind it, as above.  Only the state inputs `in` can be shared:
 *                      perturbations, forcings, the trajectory fluxes, every result and qsat_out stay per member.
 *                      A set bit on a NULL entry of `in` (in[NL_IN_QSAT] of the step and fused entries), or any bit
 *                      other than bits 0 .. 15 and the two below, is CLOUDSC2_E_ARG.  (Signed in the prototype, like
 *                      every integer of this header; a negative value has bits that are refused.)
 *                      CLOUDSC2_ENSS_COLUMN_MAJOR / CLOUDSC2_ENSS_MEMBER_MAJOR (at most one, CLOUDSC2_E_ARG otherwise)
 *                      choose how workgroups are dealt to (member, column block) pairs: column block * nmem + member - the
 *                      workgroups that read one column block of a shared field are neighbours in dispatch order - or
 *                      member * ceil(nx / 256) + column block as in the entries above.  Neither bit: the library's
 *                      default (member-major; docs/TUNING_LOG.md 3.27).  The results do not depend on the order.
 *   eta_member_stride  0: one `eta` for all members; >= nz + 1: member m's level vector starts m * eta_member_stride
 *                      ELEMENTS behind `eta`; anything else is CLOUDSC2_E_ARG.
 *       shared-state entry          ensemble entry               kernel reported by cloudsc2_last_kernel
 *       cloudsc2_nl_enss_*          cloudsc2_nl_ens_*            cs2::nl_enss_kernel
 *       cloudsc2_nl_fused_enss_*    cloudsc2_nl_fused_ens_*      cs2::nl_enss_kernel<saturation>
 *       cloudsc2_tl_enss_*          cloudsc2_tl_ens_*            cs2::tl_enss_kernel
 *       cloudsc2_tl_step_enss_*     cloudsc2_tl_step_ens_*       cs2::tl_enss_step_kernel
 *       cloudsc2_ad_enss_*          cloudsc2_ad_ens_*            cs2::ad_enss_kernel
 *       cloudsc2_ad_step_enss_*     cloudsc2_ad_step_ens_*       cs2::ad_enss_step_kernel
 * Every rule of the ensemble entry holds (the 4 GiB bound is per member, as there).  In addition a written field - a result,
 * out / out_i / out_adj, or qsat_out - whose extent in ANY member overlaps a shared input, or the per-member eta rows, is refused (CLOUDSC2_E_ARG): every
 * member reads that input for the whole launch.  With shared_mask = 0 and eta_member_stride = 0 the results are those of
 * the ensemble entry bit for bit; in general member m's results are what the single entry writes for member m's state (its
 * own fields and the shared ones) and member m's `eta`.  The adjoint entries write PER-MEMBER adjoints of shared inputs too
 * (out_adj is batched): the adjoint of the shared field itself is their sum over the members, left to the caller.
 * Not available for the evaporation-switch ensembles (cloudsc2_ad_evap*_ens_*) and members times directions
 * (cloudsc2_ad_multi*_ens_*): materialise the members for those. */
#define CLOUDSC2_ENSS_COLUMN_MAJOR (INT64_C(1) << 32)
#define CLOUDSC2_ENSS_MEMBER_MAJOR (INT64_C(1) << 33)
int32_t cloudsc2_nl_enss_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                             const double* const* in, const double* eta, double* const* out, double dt, void* stream,
                             int32_t nmem, int64_t member_stride, int64_t shared_mask, int64_t eta_member_stride);
int32_t cloudsc2_nl_enss_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                             const float* const* in, const float* eta, float* const* out, double dt, void* stream,
                             int32_t nmem, int64_t member_stride, int64_t shared_mask, int64_t eta_member_stride);
int32_t cloudsc2_nl_fused_enss_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                   const double* const* in, const double* const* in_i, double pf, double* qsat_out,
                                   const double* eta, double* const* out, double dt, void* stream,
                                   int32_t nmem, int64_t member_stride, int64_t shared_mask, int64_t eta_member_stride);
int32_t cloudsc2_nl_fused_enss_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                   const float* const* in, const float* const* in_i, double pf, float* qsat_out,
                                   const float* eta, float* const* out, double dt, void* stream,
                                   int32_t nmem, int64_t member_stride, int64_t shared_mask, int64_t eta_member_stride);
int32_t cloudsc2_tl_enss_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                             const double* const* in, const double* const* in_i, const double* zero_line,
                             const double* eta, double* const* out, double* const* out_i, double dt, void* stream,
                             int32_t nmem, int64_t member_stride, int64_t shared_mask, int64_t eta_member_stride);
int32_t cloudsc2_tl_enss_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                             const float* const* in, const float* const* in_i, const float* zero_line,
                             const float* eta, float* const* out, float* const* out_i, double dt, void* stream,
                             int32_t nmem, int64_t member_stride, int64_t shared_mask, int64_t eta_member_stride);
int32_t cloudsc2_tl_step_enss_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                  const double* const* in, const double* const* in_i, const double* zero_line,
                                  const double* eta, double* const* out, double* const* out_i, double dt, void* stream,
                                  int32_t nmem, int64_t member_stride, int64_t shared_mask, int64_t eta_member_stride);
int32_t cloudsc2_tl_step_enss_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                  const float* const* in, const float* const* in_i, const float* zero_line,
                                  const float* eta, float* const* out, float* const* out_i, double dt, void* stream,
                                  int32_t nmem, int64_t member_stride, int64_t shared_mask, int64_t eta_member_stride);
int32_t cloudsc2_ad_enss_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                             const double* const* in, const double* const* in_adj, const double* zero_line,
                             const double* eta, const double* traj_fplsl, const double* traj_fplsn,
                             double* const* out_adj, double dt, void* stream, int32_t nmem, int64_t member_stride,
                             int64_t shared_mask, int64_t eta_member_stride);
int32_t cloudsc2_ad_enss_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                             const float* const* in, const float* const* in_adj, const float* zero_line,
                             const float* eta, const float* traj_fplsl, const float* traj_fplsn,
                             float* const* out_adj, double dt, void* stream, int32_t nmem, int64_t member_stride,
                             int64_t shared_mask, int64_t eta_member_stride);
int32_t cloudsc2_ad_step_enss_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                  const double* const* in, const double* const* in_adj, const double* zero_line,
                                  const double* eta, const double* traj_fplsl, const double* traj_fplsn,
                                  double* const* out_adj, double dt, void* stream, int32_t nmem, int64_t member_stride,
                                  int64_t shared_mask, int64_t eta_member_stride);
int32_t cloudsc2_ad_step_enss_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                  const float* const* in, const float* const* in_adj, const float* zero_line,
                                  const float* eta, const float* traj_fplsl, const float* traj_fplsn,
                                  float* const* out_adj, double dt, void* stream, int32_t nmem, int64_t member_stride,
                                  int64_t shared_mask, int64_t eta_member_stride);

/* ---- ENSEMBLES WITH THE EVAPORATION BLOCK (BUILD EXTENSIONS): cloudsc2_ad_evap_* and cloudsc2_ad_evap_step_* for `nmem`
 * members in one launch, one cotangent per member.  Arguments are those of the single entry, `cover` and `cover_ready` in
 * front of `stream` included, followed by `nmem` and `member_stride` as in every ensemble entry above:
 *       ensemble entry               single entry               kernel reported by cloudsc2_last_kernel
 *       cloudsc2_ad_evap_ens_*       cloudsc2_ad_evap_*         cs2::ad_cover_ens_kernel
 *       cloudsc2_ad_evap_step_ens_*  cloudsc2_ad_evap_step_*    cs2::ad_cover_ens_step_kernel
 * Everything is batched, `cover` too: it is member-major with the call's lev_stride and the call's ONE member_stride, member
 * m's level k = the cover entering level k of member m; level nz of no member is touched.  `eta`, `dt`, the switches and the
 * zero line are shared; an absent forcing is read from the zero line by every member.  cover_ready holds for all members.
 * One workgroup serves one column block of one member and runs both sweeps for its columns: the grid is nmem * ceil(nx / 256)
 * workgroups, none depends on another.  The member's base is added to the field pointers as a 64-bit scalar, the lanes' byte
 * offsets stay 32-bit; elements between the members are not touched.
 * Refused on the host, before any launch - what the single evaporation entries and what the ensemble adjoints refuse:
 * cover == NULL, nmem < 1, member_stride < (nz+1) * lev_stride (CLOUDSC2_E_ARG); a `cover` of which any member overlaps any
 * member of another field of the call, the zero line or `eta` (CLOUDSC2_E_ARG: sweep 1 writes it while the other is read);
 * NEITHER LEVAPLS2 nor LDRAIN1D (CLOUDSC2_E_UNSUPPORTED; the message names cloudsc2_ad_ens_* / cloudsc2_ad_step_ens_*);
 * the step entry without LPHYLIN (CLOUDSC2_E_UNSUPPORTED) or with out_adj[NL_IN_QSAT] (CLOUDSC2_E_ARG); no adjoint wanted
 * (CLOUDSC2_E_ARG); one member of a field at 4 GiB or more, or more than 2^31 - 1 workgroups (CLOUDSC2_E_UNSUPPORTED).
 * nx == 0 is a successful no-op.
 * Words moved per level and column: the single entry's, per member - sweep 1 reads 16 (step: 15) + 2 and writes 1; sweep 2
 * moves 16 (15) + 2 + 1 + (present in_adj) + (wanted out_adj).  With cover_ready sweep 1's 19 (18) drop out.
 * Every member of every written adjoint and of `cover` equals what the single entry writes for that member alone, to
 * rounding (each kernel contracts the level functions itself).  Members times directions with the evaporation block: no such entry
 * (cloudsc2_ad_multi_ens_* below covers the driver switches). */
int32_t cloudsc2_ad_evap_ens_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                 const double* const* in, const double* const* in_adj, const double* zero_line,
                                 const double* eta, const double* traj_fplsl, const double* traj_fplsn,
                                 double* const* out_adj, double dt, double* cover, int32_t cover_ready, void* stream,
                                 int32_t nmem, int64_t member_stride);
int32_t cloudsc2_ad_evap_ens_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                 const float* const* in, const float* const* in_adj, const float* zero_line,
                                 const float* eta, const float* traj_fplsl, const float* traj_fplsn,
                                 float* const* out_adj, double dt, float* cover, int32_t cover_ready, void* stream,
                                 int32_t nmem, int64_t member_stride);
int32_t cloudsc2_ad_evap_step_ens_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                      const double* const* in, const double* const* in_adj, const double* zero_line,
                                      const double* eta, const double* traj_fplsl, const double* traj_fplsn,
                                      double* const* out_adj, double dt, double* cover, int32_t cover_ready, void* stream,
                                      int32_t nmem, int64_t member_stride);
int32_t cloudsc2_ad_evap_step_ens_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                      const float* const* in, const float* const* in_adj, const float* zero_line,
                                      const float* eta, const float* traj_fplsl, const float* traj_fplsn,
                                      float* const* out_adj, double dt, float* cover, int32_t cover_ready, void* stream,
                                      int32_t nmem, int64_t member_stride);

/* ---- ENSEMBLE JACOBIANS (BUILD EXTENSIONS): cloudsc2_ad_multi_* and cloudsc2_ad_multi_step_* for `nmem` MEMBERS in one launch
 * - members times directions: a block of Jacobian rows for every member of an ensemble (`vmap(jacrev(f))` over stacked
 * states), several observation functionals per member.  Arguments are those of the multi entry, followed by:
 *   nmem               number of members, >= 1 (CLOUDSC2_E_ARG otherwise);
 *   member_stride      in ELEMENTS, for in[] and the two trajectory fluxes: member m of each starts m * member_stride
 *                      elements behind the pointer.  At least (nz+1) * lev_stride (CLOUDSC2_E_ARG);
 *   in_member_stride   in ELEMENTS, for every present in_adj[f]: direction d of member m starts
 *                      m * in_member_stride + d * in_dir_stride elements behind the pointer;
 *   out_member_stride  in ELEMENTS, the same for every wanted out_adj[f] with out_dir_stride.
 *       ensemble entry                  multi entry                kernel reported by cloudsc2_last_kernel
 *       cloudsc2_ad_multi_ens_*         cloudsc2_ad_multi_*        cs2::ad_mdirs_kernel
 *       cloudsc2_ad_multi_step_ens_*    cloudsc2_ad_multi_step_*   cs2::ad_mdirs_step_kernel
 * All pointers are member 0 / direction 0.  The batches are MEMBER-MAJOR only: in_member_stride must be at least
 * (ndir-1) * in_dir_stride + (nz+1) * lev_stride and out_member_stride at least (ndir-1) * out_dir_stride + (nz+1) * lev_stride
 * (CLOUDSC2_E_ARG) - a member's directions lie inside its member stride.  `eta`, `dt`, the switches and the zero line are
 * shared by all members and directions; a field is present or absent for all of them alike.
 * Everything cloudsc2_ad_multi_* refuses is refused here, on the host and before any launch: LEVAPLS2 / LDRAIN1D
 * (CLOUDSC2_E_UNSUPPORTED), the step without LPHYLIN (CLOUDSC2_E_UNSUPPORTED) or with out_adj[NL_IN_QSAT] (CLOUDSC2_E_ARG),
 * ndir outside 1 .. CLOUDSC2_AD_MAX_DIRS (CLOUDSC2_E_ARG), an LDS demand above 160 KB (CLOUDSC2_E_UNSUPPORTED; the demand is
 * the multi entry's, it does not grow with nmem).  A field stays below 4 GiB PER MEMBER AND DIRECTION (CLOUDSC2_E_UNSUPPORTED
 * otherwise; member and direction bases are added to the field pointers as 64-bit scalars, the lanes' byte offsets are
 * 32-bit); nmem * ceil(nx / 256) workgroups must fit a one-dimensional grid, 2^31 - 1 (CLOUDSC2_E_UNSUPPORTED).  nx == 0 is a
 * successful no-op.
 * One workgroup serves one column block of one member, all directions.  Every member and direction of every written field
 * equals what the multi entry writes for that member alone, to rounding (each kernel contracts the level functions
 * itself).  Elements between members and between directions are not touched.
 * Words moved per level and column, per member: 16 (step: 15) + 2 + ndir * ((present in_adj) + (present out_adj)) - the multi
 * entry's; one launch instead of nmem. */
int32_t cloudsc2_ad_multi_ens_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                  const double* const* in, const double* const* in_adj, const double* zero_line,
                                  const double* eta, const double* traj_fplsl, const double* traj_fplsn,
                                  double* const* out_adj, double dt, void* stream,
                                  int32_t ndir, int64_t in_dir_stride, int64_t out_dir_stride,
                                  int32_t nmem, int64_t member_stride, int64_t in_member_stride, int64_t out_member_stride);
int32_t cloudsc2_ad_multi_ens_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                  const float* const* in, const float* const* in_adj, const float* zero_line,
                                  const float* eta, const float* traj_fplsl, const float* traj_fplsn,
                                  float* const* out_adj, double dt, void* stream,
                                  int32_t ndir, int64_t in_dir_stride, int64_t out_dir_stride,
                                  int32_t nmem, int64_t member_stride, int64_t in_member_stride, int64_t out_member_stride);
int32_t cloudsc2_ad_multi_step_ens_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                       const double* const* in, const double* const* in_adj, const double* zero_line,
                                       const double* eta, const double* traj_fplsl, const double* traj_fplsn,
                                       double* const* out_adj, double dt, void* stream,
                                       int32_t ndir, int64_t in_dir_stride, int64_t out_dir_stride,
                                       int32_t nmem, int64_t member_stride, int64_t in_member_stride, int64_t out_member_stride);
int32_t cloudsc2_ad_multi_step_ens_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t lev_stride,
                                       const float* const* in, const float* const* in_adj, const float* zero_line,
                                       const float* eta, const float* traj_fplsl, const float* traj_fplsn,
                                       float* const* out_adj, double dt, void* stream,
                                       int32_t ndir, int64_t in_dir_stride, int64_t out_dir_stride,
                                       int32_t nmem, int64_t member_stride, int64_t in_member_stride, int64_t out_member_stride);

#ifdef __cplusplus
}
#endif
#endif /* CLOUDSC2_HIP_H */
