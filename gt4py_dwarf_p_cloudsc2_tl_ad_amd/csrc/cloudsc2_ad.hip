// cloudsc2_ad as a hand-written CDNA4 kernel.  Restates
// /root/reference/src/cloudsc2_gt4py/physics/adjoint/_stencils/cloudsc2.py:124-996 and
// /root/reference/src/cloudsc2_gt4py/physics/adjoint/_stencils/cuadjtqs.py:22-158
// (line numbers below refer to the first file unless prefixed "cuadjtqs").
//
// GT4Py keeps ~80 trajectory temporaries of the forward computation as full 3-D fields for the
// backward computation.  Here NOTHING but the stencil's own outputs goes to HBM:
//   sweep 1 (k = 0 .. nz-1)  recomputes the NL trajectory and writes the 10 NL outputs (:146-475);
//   sweep 2 (k = nz-1 .. 0)  re-reads level k's 16 state inputs + the snow flux that entered the
//                            level (= out_fplsn[k], written by sweep 1 of the same lane), recomputes
//                            that level's local trajectory in registers and runs the adjoint
//                            statements (:479-996) on it.
// The only loop-carried trajectory values are the fluxes entering a level, and those are outputs.
// Backward carries: tmp_rfln_i, tmp_sfln_i, rfl_i/sfl_i of the level below, and daph_i/dp_i/dlu_i of
// the level below for the staggered corrections (:970-986), which are fused into the sweep.
//
// Deliberate, documented choices:
//   Q1  adjoint forcings (in_*_i) are read-only here; the reference zeroes them in place.
//   Q8  rfl_i / sfl_i of a level that does not melt read as 0 (unassigned GT4Py temporaries).
//   out_lude_i is written (=), not accumulated into prior storage contents (:526 uses -= on an
//       output the stencil never initialises; zero-initialised storage gives the same result).
//   Q4/Q5 are reproduced literally when FIX = false (the reference's behaviour): the second
//       freezing test uses the pre-adjustment t3 (:427, :577) and the adjoint of rfreeze1 tests the
//       post-adjustment t (:729).  FIX = true (Cloudsc2Params.AD_TRAJ_FIX, a build extension) uses
//       the tests of the NL/TL stencils instead, which makes AD the exact transpose of TL.
// Template flags: REG = LREGCL; EVAP = LEVAPLS2 or LDRAIN1D (evaporation block :357-394 / :635-709).
// With EVAP the precipitation cover entering a level (tmp_covptotp, :458) is a second loop-carried
// trajectory value that is NOT an output (out_covptot is 0 on levels without evaporation): sweep 1
// parks it in level k of out_mfd_i, sweep 2 reads it back before it overwrites that element.
#include "cloudsc2_ad_level.hpp"

namespace cs2 {

// Kernel arguments as ONE struct (kernarg offset 0): the field pointers are fetched from the kernarg segment at their
// point of use (KernArgs in cloudsc2_common.hpp) instead of living in - and being spilled from - SGPRs.
template <typename T>
struct ADArgs {
    Ext<T> e;
    NLK<T> kc;
    ExpK<T> xk;
    int nx, nz;
    int64_t ls;
    CPtrs<T, NL_NUM_IN> in;
    CPtrs<T, NL_NUM_OUT> adj;
    const T* eta;
    MPtrs<T, NL_NUM_OUT> out;
    MPtrs<T, NL_NUM_IN> oadj;
    T dt;
    const T* traj_l;   // TRAJ instantiation only: the rain / snow fluxes ENTERING each level (= out_fplsl / out_fplsn of a
    const T* traj_n;   // cloudsc2_nl / cloudsc2_tl call on the same state), read instead of recomputed by sweep 1
};
template <typename T>
struct ADFields : KernArgs<ADArgs<T>> {
    __device__ __forceinline__ const T* in(int i) const { return this->ka->in.p[i]; }
    __device__ __forceinline__ const T* adj(int i) const { return this->ka->adj.p[i]; }
    __device__ __forceinline__ T* out(int i) const { return this->ka->out.p[i]; }
    __device__ __forceinline__ const T* outc(int i) const { return this->ka->out.p[i]; }
    __device__ __forceinline__ T* oadj(int i) const { return this->ka->oadj.p[i]; }
    __device__ __forceinline__ const T* oadjc(int i) const { return this->ka->oadj.p[i]; }
    __device__ __forceinline__ const T* traj_l() const { return this->ka->traj_l; }
    __device__ __forceinline__ const T* traj_n() const { return this->ka->traj_n; }
};

// fp32 without the evaporation block: three waves per SIMD (<= 168 VGPRs) is what the LDS parking was built for (+4.7 %,
// DESIGN 3.5); r03's two extra raw forcing words took the unconstrained allocation to 170 VGPRs = two waves, so it is asked for.
// BIG: 64-bit byte offsets (fields of 4 GiB and more, see offset_t in cloudsc2_common.hpp).
// TRAJ (BUILD EXTENSION, C ABI cloudsc2_ad_from_trajectory_*): the symmetry test calls cloudsc2_tl and then cloudsc2_ad on
// the same state (adjoint/validation.py:135-151), and the only loop-carried trajectory values sweep 2 needs from sweep 1
// are the two precipitation fluxes entering each level - which the TL call has just written as out_fplsl / out_fplsn.
// With TRAJ the kernel skips sweep 1 (no NL outputs are written) and reads those two fields from `traj_l` / `traj_n`:
// 44 words per level and column instead of 70.  Without the evaporation block only (its parked cover has no such source).
template <typename T, bool REG, bool FIX, bool EVAP, bool BIG = false, bool TRAJ = false>
__global__ void __launch_bounds__(kColBlock, (sizeof(T) == 4 && !EVAP) ? 3 : 1)
ad_kernel(const ADArgs<T> A) {
    Ext<T> e = A.e;
    NLK<T> kc = A.kc;
    ExpK<T> xk = A.xk;
    const int nx = A.nx, nz = A.nz;
    const int64_t ls = A.ls;
    const T* __restrict__ eta = A.eta;
    T dt = A.dt;
    ADFields<T> F;
    const auto F_in = [&](int i) { return F.in(i); };
    extern __shared__ __align__(16) unsigned char smem_raw[];
    T* s_eta = reinterpret_cast<T*>(smem_raw);
    T* s_scalm = s_eta + (nz + 1);
    int klo, khi;
    build_level_table<T>(eta, nz, e, s_eta, s_scalm, klo, khi);
    if constexpr (sizeof(T) == 8) {
        // fp64 constants of the level loops -> VGPRs (see pin_vgpr in cloudsc2_common.hpp)
        pin_vgprs(e.RCPD, e.RLSTT, e.RLVTT, e.R4LES, e.R4IES, e.RTT, e.R3IES, e.R3LES, e.R2ES, e.ZQMAX, e.RETV, e.R5LES,
                  e.R5IES, e.RG, e.RD, kc.rdt, kc.cons2, kc.rRD, kc.rRCPD, dt);
        pin_expk(xk);
    }

    const int gcol = xcd_block() * kColBlock + threadIdx.x;
    // kADPark: this lane's parking slots follow the level table (8-byte aligned)
    T* const park_lds = s_scalm + (nz + 1) + threadIdx.x;
    (void)park_lds;
    if (gcol >= nx) return;  // no later workgroup barrier: whole lanes may retire
    using O = offset_t<BIG>;
#if CS2_AD_DIAG == 2
    const O lsb = nz < 0 ? O(ls) : O(0);   // diagnostics only (wrong results): every level reads and writes level 0 -
#else                                                  // cache-resident rows, the kernel's time without HBM
    const O lsb = O(ls) * O(sizeof(T));
#endif
    const O colb = O(gcol) * O(sizeof(T));

    const T trpaus = trpaus_prescan<T, false, O>(F.in(NL_IN_T), F.in(NL_IN_TND_CML_T), lsb, colb, dt, s_eta, klo, khi);
    const CrhCol<T> crh = crh_setup<T>(trpaus);

    static_assert(!(TRAJ && EVAP), "the trajectory variant has no source for the evaporation block's parked cover");
    // ---------------- sweep 1: trajectory + NL outputs (:146-475)
    const T aph_s = EVAP ? ldg(F.in(NL_IN_APH), O(nz) * lsb + colb) : T(1.0);
#define park F.oadj(NL_IN_MFD)  // EVAP: level k holds the cover entering level k until sweep 2 overwrites it
    if constexpr (!TRAJ) {
        stg(F.out(NL_OUT_FPLSL), colb, T(0.0));
        stg(F.out(NL_OUT_FPLSN), colb, T(0.0));
        stg(F.out(NL_OUT_FHPSL), colb, T(0.0));
        stg(F.out(NL_OUT_FHPSN), colb, T(0.0));
        T rfl = T(0.0), sfl = T(0.0), covptot = T(0.0);
        T aph_k = ldg(F.in(NL_IN_APH), colb);
        O o = colb;
        LevelIn<T> xa = load_level<T>(F_in, lsb, o);
        for (int k = 0; k < nz; ++k) {
            F.fresh();
            LevelIn<T> xn = xa;
            if (k + 1 < nz) xn = load_level<T>(F_in, lsb, o + lsb);
            ADTraj<T> r;
            ad_forward<T, FIX, EVAP>(e, kc, xk, xa, aph_k, k, s_eta[k], s_scalm[k], crh, dt, rfl, sfl, covptot, aph_s,
                                     r);
            if constexpr (EVAP) stg(park, o, covptot);
            covptot = r.covptot;
            stg(F.out(NL_OUT_CLC), o, r.out_clc);
            stg(F.out(NL_OUT_COVPTOT), o, r.out_covptot);
            stg(F.out(NL_OUT_TND_Q), o, r.tnd_q);
            stg(F.out(NL_OUT_TND_T), o, r.tnd_t);
            stg(F.out(NL_OUT_TND_QL), o, r.tnd_ql);
            stg(F.out(NL_OUT_TND_QI), o, r.tnd_qi);
            stg(F.out(NL_OUT_FPLSL), o + lsb, r.rfln);
            stg(F.out(NL_OUT_FPLSN), o + lsb, r.sfln);
            stg(F.out(NL_OUT_FHPSL), o + lsb, -r.rfln * e.RLVTT);
            stg(F.out(NL_OUT_FHPSN), o + lsb, -r.sfln * e.RLSTT);
            rfl = r.rfln;
            sfl = r.sfln;
            aph_k = xa.aph1;
            xa = xn;
            o += lsb;
        }
    }   // !TRAJ

    // ---------------- sweep 2: adjoint (:479-996), k = nz-1 .. 0
    ADBack<T> b = zero_back<T>(aph_s);
    {
        int k = nz - 1;
        O o = O(k) * lsb + colb;
        LevelIn<T> xa = load_level<T>(F_in, lsb, o);
        ADForce<T> fa = ad_load_force<T, EVAP>(F, e, lsb, o);
        T aph_k = ldg(F.in(NL_IN_APH), o);
        T sfl = ldg(TRAJ ? F.traj_n() : F.outc(NL_OUT_FPLSN), o);
        T rfl = ldg(TRAJ ? F.traj_l() : F.outc(NL_OUT_FPLSL), o);
        T cov = EVAP ? ldg(F.oadjc(NL_IN_MFD), o) : T(0.0);
        for (; k >= 0; --k) {
            F.fresh();
            LevelIn<T> xn = xa;
            ADForce<T> fn = fa;
            T aph_n = aph_k, sfl_n = sfl, rfl_n = rfl, cov_n = cov;
            if (k > 0) {
                const O om = o - lsb;
                xn = load_level<T>(F_in, lsb, om);
                xn.aph1 = aph_k;   // aph[k]: already here as this level's upper half level (the load above is dropped)
                fn = ad_load_force<T, EVAP>(F, e, lsb, om);
                aph_n = ldg(F.in(NL_IN_APH), om);
                sfl_n = ldg(TRAJ ? F.traj_n() : F.outc(NL_OUT_FPLSN), om);
                rfl_n = ldg(TRAJ ? F.traj_l() : F.outc(NL_OUT_FPLSL), om);
                if constexpr (EVAP) cov_n = ldg(F.oadjc(NL_IN_MFD), om);
            }
            ADTraj<T> r;
            ad_forward<T, FIX, EVAP>(e, kc, xk, xa, aph_k, k, s_eta[k], s_scalm[k], crh, dt, rfl, sfl, cov, aph_s, r);
            if constexpr (kADPark<T>) ad_park<T>(park_lds, r);
            const ADOut<T> a = ad_backward<T, REG, FIX, EVAP>(e, kc, xa, k, s_scalm[k], dt, sfl, r, fa, b, park_lds);
            stg(F.oadj(NL_IN_AP), o, a.ap);
            stg(F.oadj(NL_IN_T), o, a.t);
            stg(F.oadj(NL_IN_Q), o, a.q);
            stg(F.oadj(NL_IN_QL), o, a.ql);
            stg(F.oadj(NL_IN_QI), o, a.qi);
            stg(F.oadj(NL_IN_QSAT), o, a.qsat);
            stg(F.oadj(NL_IN_LUDE), o, a.lude);
            stg(F.oadj(NL_IN_MFD), o, a.mfd);
            stg(F.oadj(NL_IN_MFU), o, a.mfu);
            stg(F.oadj(NL_IN_SUPSAT), o, dt * a.q);           // :992 (Q7, literal)
            stg(F.oadj(NL_IN_TND_CML_T), o, dt * a.t);        // :993-996
            stg(F.oadj(NL_IN_TND_CML_Q), o, dt * a.q);
            stg(F.oadj(NL_IN_TND_CML_QL), o, dt * a.ql);
            stg(F.oadj(NL_IN_TND_CML_QI), o, dt * a.qi);
            stg(F.oadj(NL_IN_APH), o + lsb, a.aph1);
            stg(F.oadj(NL_IN_LU), o + lsb, a.lu1);
            xa = xn;
            fa = fn;
            aph_k = aph_n;
            sfl = sfl_n;
            rfl = rfl_n;
            cov = cov_n;
            o -= lsb;
        }
    }
    if constexpr (EVAP) {  // :970-971: out_aph_i[nz] also receives the accumulated tmp_aph_s_i
        const O on = O(nz) * lsb + colb;
        stg(F.oadj(NL_IN_APH), on, ldg(F.oadjc(NL_IN_APH), on) + b.aph_s_i);
    }
    // :982-986 top half level
    stg(F.oadj(NL_IN_APH), colb, b.daph_i - b.dp_i);
    stg(F.oadj(NL_IN_LU), colb, T(0.0));
#undef park
}

// traj_l / traj_n != nullptr: the trajectory variant (TRAJ above); `out` may then be nullptr (nothing of it is touched).
template <typename T>
int launch_ad(const Cloudsc2Params& p, int nx, int nz, int64_t ls, const T* const* in, const T* const* in_adj,
              const T* eta, T* const* out, T* const* out_adj, double dt, hipStream_t stream, const T* traj_l,
              const T* traj_n) {
    const bool traj = traj_l != nullptr && traj_n != nullptr;
    const bool evap = evap_on(p);
    const Ext<T> e = make_ext<T>(p);
    const auto ci = pack_ptrs<CPtrs<T, NL_NUM_IN>>(in);
    const auto ca = pack_ptrs<CPtrs<T, NL_NUM_OUT>>(in_adj);
    const auto co = pack_ptrs<MPtrs<T, NL_NUM_OUT>>(out);
    const auto coa = pack_ptrs<MPtrs<T, NL_NUM_IN>>(out_adj);
    const dim3 grid((nx + kColBlock - 1) / kColBlock);
    const size_t smem = 2 * size_t(nz + 1) * sizeof(T) + (kADPark<T> ? size_t(CS2_AD_PARK_COUNT) * kColBlock * sizeof(T) : 0);
    const T tdt = static_cast<T>(dt);
    const NLK<T> kc = make_nlk<T>(p, dt, evap);
    const ExpK<T> xk = make_expk<T>();
    const bool big = !fits_u32_offsets<T>(nz, ls);
    // the trajectory variant: driver switches, 32-bit offsets.  (Refused in front of the launch tail's device look-up, which
    // it used to follow: both refuse without a side effect, and the entry that leads here checks the same before it calls.)
    if (traj && (evap || big)) return -2;
    const ADArgs<T> args = {e, kc, xk, nx, nz, ls, ci, ca, eta, co, coa, tdt, traj_l, traj_n};
    const Launch l{grid, smem, stream, traj ? "cs2::ad_kernel<trajectory>" : big ? "cs2::ad_kernel<big>" : "cs2::ad_kernel"};
    return with_flags(
        [&](auto REG, auto FIX, auto TRAJ, auto EVAP, auto BIG) {
            if constexpr (TRAJ && (EVAP || BIG)) return -2;   // refused above: no such instantiation
            else return launch_tail<ad_kernel<T, REG, FIX, EVAP, BIG, TRAJ>>(l, args);
        },
        p.LREGCL != 0, p.AD_TRAJ_FIX != 0, traj, evap, big);
}

template int launch_ad<double>(const Cloudsc2Params&, int, int, int64_t, const double* const*, const double* const*,
                               const double*, double* const*, double* const*, double, hipStream_t, const double*,
                               const double*);
template int launch_ad<float>(const Cloudsc2Params&, int, int, int64_t, const float* const*, const float* const*,
                              const float*, float* const*, float* const*, double, hipStream_t, const float*, const float*);

// ------------------------------------------------------------------------------------------------------------------
// Masked adjoint (BUILD EXTENSION, C ABI cloudsc2_ad_masked_*): the vector-Jacobian product as an automatic-differentiation
// framework asks for it - forcing on a few NL outputs, adjoints of a few inputs.  Sweep 2 of ad_kernel<TRAJ> (same
// ad_forward / ad_backward, same prefetch of one level, same parking) in which
//   * an ABSENT FORCING is still loaded - every load of a level is issued unconditionally, so hipcc's wait-count insertion
//     keeps an exact count of the loads in flight and the wait for level k-1's words never reaches the prefetch of level
//     k-2 just issued (a wave-uniform branch around a load - `p ? ldg(p, o) : 0` - loses that count, and with it the only
//     memory-level parallelism one wave per SIMD has).  What differs is WHERE it reads: the launcher has replaced the
//     field's pointer by the caller's zero line and the lane's offset becomes lane * sizeof(T) (one v_cndmask on a
//     wave-uniform bit of `have`).  Every wave reads the same 512 B, which stay in cache: no HBM word moves;
//   * an UNWANTED ADJOINT is not stored: a wave-uniform branch on a bit of `want` around the store.  The store count of a
//     level is then unknown to hipcc, so the wait for the next level's words also covers the stores issued since those
//     words were requested; the kernel therefore issues a level's stores one iteration late (see the loop), where they
//     have a whole level's arithmetic to complete before that wait.
// The words the level functions see are those of the dense call with zero fields, so the adjoints that are written are
// the trajectory variant's bit for bit.  Driver switches and 32-bit offsets only, as ad_kernel<TRAJ>.
// The same call for every MEMBER of an ensemble (ad_ens_kernel / ad_ens_step_kernel, C ABI cloudsc2_ad_ens_* /
// cloudsc2_ad_step_ens_*): see ens_block.  ADEnsFields is ADMaskedFields moved to one member: the member's base `mb`
// (elements; wave-uniform) is added to the field pointer as a 64-bit scalar, the way ad_dirs_sweep adds the direction base;
// an absent forcing keeps the zero line's pointer (the line is 512 bytes long).  An unwanted adjoint's pointer is never used.
// (ADEnsArgs / ADEnsFields: cloudsc2_ad_level.hpp - the cover kernels' ensemble forms in cloudsc2_ad_evap.hip use them too.)

// The sweep of ad_masked_kernel and of ad_step_kernel (one copy).  STEP: the adjoint of `saturation` is fused in (C ABI
// cloudsc2_ad_step_*).  in_qsat is not read: the level's qsat is saturation_point's value of the level's t and ap words
// (LPHYLIN form, what cloudsc2_nl_fused_* computes).  The level's qsat adjoint (ADOut::qsat) is not stored but folded into
// the t and ap adjoints as g_t * qsat_adj and g_ap * qsat_adj.  The two exponentials of g_t / g_ap stay out of ad_backward's
// live range (the fp64 instantiation already parks trajectory words in LDS to stay within 256 VGPRs): the level's t and ap
// (`pt`, `pap`: two words) are kept beside its adjoints and the derivative is formed where those are stored, one iteration
// late and before the next level's arithmetic starts.
// ENS: one member of an ensemble per workgroup (`g`: EnsGeom; the field pointers are ADEnsFields').
// G = EnssGeom: the members share part of their state and may each have an `eta` (C ABI cloudsc2_ad_enss_* /
// cloudsc2_ad_step_enss_*; see EnssGeom).  The member is decoded in front of the level table, which is built from the member's
// own level vector; the field pointers are ADEnssFields'.  Nothing else differs: the level loop is the ensemble form's.
template <typename T, bool REG, bool FIX, bool STEP, bool ENS = false, typename G = EnsGeom>
__device__ __forceinline__ void ad_masked_sweep(const ADMaskedArgs<T>& A, const G g = G{}) {
    constexpr bool SH = kSharedGeom<G>;
    static_assert(ENS || !SH, "shared state is an ensemble form");
    Ext<T> e = A.e;
    NLK<T> kc = A.kc;
    ExpK<T> xk = A.xk;
    const int nx = A.nx, nz = A.nz;
    const int64_t ls = A.ls;
    const T* __restrict__ eta = A.eta;
    T dt = A.dt;
    const uint32_t have = A.have, want = A.want;
    typename std::conditional<SH, ADEnssFields<T>, typename std::conditional<ENS, ADEnsFields<T>, ADMaskedFields<T>>::type>::type F;
    const auto F_in = [&](int i) { return F.in(i); };
    extern __shared__ __align__(16) unsigned char smem_raw[];
    T* s_eta = reinterpret_cast<T*>(smem_raw);
    T* s_scalm = s_eta + (nz + 1);
    int klo, khi;
    int member = 0, cblock = 0;
    if constexpr (SH) {
        cblock = enss_block(g, member);
        eta += member * g.eta_ms;
    }
    build_level_table<T>(eta, nz, e, s_eta, s_scalm, klo, khi);
    if constexpr (sizeof(T) == 8) {
        pin_vgprs(e.RCPD, e.RLSTT, e.RLVTT, e.R4LES, e.R4IES, e.RTT, e.R3IES, e.R3LES, e.R2ES, e.ZQMAX, e.RETV, e.R5LES,
                  e.R5IES, e.RG, e.RD, kc.rdt, kc.cons2, kc.rRD, kc.rRCPD, dt);
        pin_expk(xk);
    }

    int gcol;
    if constexpr (ENS) {
        if constexpr (!SH) cblock = ens_block(g.bpm, member);
        gcol = cblock * kColBlock + threadIdx.x;
        F.mb = member * g.ms;
        F.have = have;
        if constexpr (SH) F.sh = g.shared;
    } else {
        gcol = xcd_block() * kColBlock + threadIdx.x;
    }
    T* const park_lds = s_scalm + (nz + 1) + threadIdx.x;
    (void)park_lds;
    if (gcol >= nx) return;  // no later workgroup barrier: whole lanes may retire
    using O = uint32_t;
    const O lsb = O(ls) * O(sizeof(T));
    const O colb = O(gcol) * O(sizeof(T));
    const O zo = O(threadIdx.x & (kWave - 1)) * O(sizeof(T));   // this lane's word of the zero line

    const T trpaus = trpaus_prescan<T, false, O>(F.in(NL_IN_T), F.in(NL_IN_TND_CML_T), lsb, colb, dt, s_eta, klo, khi);
    const CrhCol<T> crh = crh_setup<T>(trpaus);

    ADBack<T> b = zero_back<T>(T(1.0));
    // ONE loop, k = nz .. -1, and nothing of a level outside it: iteration k requests level k-1's words, stores level k+1's
    // adjoints and computes level k (the first iteration only requests, the last only stores).
    //   * A level's adjoints are stored ONE ITERATION LATE, right behind the next prefetch: with the store count unknown,
    //     the wait for level k-1's words (requested before level k is computed, first read after it) covers every
    //     operation issued since - stores included.  Stores issued behind level k's arithmetic would be waited for at
    //     their full latency on every level; stores issued before it have long completed by then.
    //   * No prologue batch and no epilogue stores: hipcc lays such blocks out around the loop as it pleases, and
    //     check_ring_isa.check_prefetch_distance reads every backward branch as a loop.
    O o = O(nz) * lsb + colb, po = o;
    ADOut<T> pa = zero_out<T>();
    LevelIn<T> xa = zero_level<T>();
    ADForce<T> fa = zero_force<T>();
    T aph_k = ldg(F.in(NL_IN_APH), o), sfl = T(0.0), rfl = T(0.0);   // aph[nz]: level nz-1's lower half level
    T pt = T(273.0), pap = T(1.0e5);   // STEP: t and ap of the level whose adjoints `pa` holds
    for (int k = nz; k >= -1; --k) {
        F.fresh();
        LevelIn<T> xn = xa;
        ADForce<T> fn = fa;
        T aph_n = aph_k, sfl_n = sfl, rfl_n = rfl;
        if (k > 0) {
            const O om = o - lsb;
            xn = load_level<T>(F_in, lsb, om, STEP);
            xn.aph1 = aph_k;   // aph[k]: already here as this level's upper half level
            fn = ad_load_force_masked<T>(F, have, lsb, om, zo);
            aph_n = ldg(F.in(NL_IN_APH), om);
            sfl_n = ldg(F.traj_n(), om);
            rfl_n = ldg(F.traj_l(), om);
        }
        if (k < nz - 1) {
            if constexpr (STEP) {
                const SatD<T> s = saturation_point_d<T, 0>(e, xk, pt, pap);
                ad_store_masked<T, true>(F, want, lsb, po, dt, pa, s.g_ap * pa.qsat, s.g_t * pa.qsat);
            } else {
                ad_store_masked<T>(F, want, lsb, po, dt, pa);
            }
        }
        if (k >= 0 && k < nz) {
            if constexpr (STEP) xa.qsat = saturation_point<T, 0>(e, xk, xa.t, xa.ap);
            ADTraj<T> r;
            ad_forward<T, FIX, false>(e, kc, xk, xa, aph_k, k, s_eta[k], s_scalm[k], crh, dt, rfl, sfl, T(0.0), T(1.0), r);
            if constexpr (kADPark<T>) ad_park<T>(park_lds, r);
            pa = ad_backward<T, REG, FIX, false>(e, kc, xa, k, s_scalm[k], dt, sfl, r, fa, b, park_lds);
            po = o;
            if constexpr (STEP) {
                pt = xa.t;
                pap = xa.ap;
            }
        }
        xa = xn;
        fa = fn;
        aph_k = aph_n;
        sfl = sfl_n;
        rfl = rfl_n;
        o -= lsb;
    }
    // :982-986 top half level
    if (want >> NL_IN_APH & 1u) stg(F.oadj(NL_IN_APH), colb, b.daph_i - b.dp_i);
    if (want >> NL_IN_LU & 1u) stg(F.oadj(NL_IN_LU), colb, T(0.0));
}

template <typename T, bool REG, bool FIX>
__global__ void __launch_bounds__(kColBlock, sizeof(T) == 4 ? 3 : 1)
ad_masked_kernel(const ADMaskedArgs<T> A) {
    ad_masked_sweep<T, REG, FIX, false>(A);
}

// cloudsc2_ad_masked + the adjoint of `saturation` in one launch (BUILD EXTENSION, C ABI cloudsc2_ad_step_*): see
// ad_masked_sweep
template <typename T, bool REG, bool FIX>
__global__ void __launch_bounds__(kColBlock, sizeof(T) == 4 ? 3 : 1)
ad_step_kernel(const ADMaskedArgs<T> A) {
    ad_masked_sweep<T, REG, FIX, true>(A);
}

// ad_masked_kernel / ad_step_kernel for the members of an ensemble, one launch (BUILD EXTENSION, C ABI cloudsc2_ad_ens_* /
// cloudsc2_ad_step_ens_*): see ADEnsArgs
template <typename T, bool REG, bool FIX>
__global__ void __launch_bounds__(kColBlock, sizeof(T) == 4 ? 3 : 1)
ad_ens_kernel(const ADEnsArgs<T> A) {
    ad_masked_sweep<T, REG, FIX, false, true>(A.m, A.g);
}

template <typename T, bool REG, bool FIX>
__global__ void __launch_bounds__(kColBlock, sizeof(T) == 4 ? 3 : 1)
ad_ens_step_kernel(const ADEnsArgs<T> A) {
    ad_masked_sweep<T, REG, FIX, true, true>(A.m, A.g);
}

// ad_ens_kernel / ad_ens_step_kernel for members that share part of their state (BUILD EXTENSION, C ABI cloudsc2_ad_enss_* /
// cloudsc2_ad_step_enss_*): see EnssGeom
template <typename T, bool REG, bool FIX>
__global__ void __launch_bounds__(kColBlock, sizeof(T) == 4 ? 3 : 1)
ad_enss_kernel(const ADEnsArgs<T, EnssGeom> A) {
    ad_masked_sweep<T, REG, FIX, false, true, EnssGeom>(A.m, A.g);
}

template <typename T, bool REG, bool FIX>
__global__ void __launch_bounds__(kColBlock, sizeof(T) == 4 ? 3 : 1)
ad_enss_step_kernel(const ADEnsArgs<T, EnssGeom> A) {
    ad_masked_sweep<T, REG, FIX, true, true, EnssGeom>(A.m, A.g);
}


// The caller (cloudsc2_capi.hip) has refused the evaporation switches and fields of 4 GiB and more.  kStep: ad_step_kernel
// (in[NL_IN_QSAT] is not read, out_adj[NL_IN_QSAT] is NULL).  kEns: the ensemble form (ad_ens_kernel /
// ad_ens_step_kernel) - every field pointer is member 0's, member m lies m * ms elements behind it; the caller has checked
// nmem and ms.  kShared (with kEns): ad_enss_kernel / ad_enss_step_kernel - the geometry is enss_geom's.
template <typename T>
int launch_ad_masked(const ADCall<T>& c) {
    if (evap_on(*c.p) || !fits_u32_offsets<T>(c.nz, c.ls)) return -2;
    const bool step = c.is(kStep);
    const int nmem = c.is(kEns) ? c.members.nmem : 0;
    if (c.is(kShared) && nmem < 1) return -1;
    ADEnsArgs<T> ens;
    const ADMaskedArgs<T>& args = ens.m = fill_ad_masked_args<T>(c);
    const int bpm = (c.nx + kColBlock - 1) / kColBlock;
    const dim3 grid(bpm);
    const size_t smem = 2 * size_t(c.nz + 1) * sizeof(T) + (kADPark<T> ? size_t(CS2_AD_PARK_COUNT) * kColBlock * sizeof(T) : 0);
    if (nmem > 0 && int64_t(nmem) * bpm > kMaxGrid) return -2;
    ens.g.ms = c.members.ms; ens.g.bpm = bpm;
    const dim3 egrid(unsigned(nmem > 0 ? nmem : 1) * unsigned(bpm));
    return with_flags(
        [&](auto REG, auto FIX, auto STEP, auto ENS, auto SH) {
            if constexpr (ENS && SH) {
                constexpr auto kern = STEP ? ad_enss_step_kernel<T, REG, FIX> : ad_enss_kernel<T, REG, FIX>;
                const ADEnsArgs<T, EnssGeom> enss = {args, enss_geom(c.members, bpm)};
                return launch_tail<kern>({egrid, smem, c.stream, step ? "cs2::ad_enss_step_kernel" : "cs2::ad_enss_kernel"}, enss);
            } else if constexpr (ENS) {
                constexpr auto kern = STEP ? ad_ens_step_kernel<T, REG, FIX> : ad_ens_kernel<T, REG, FIX>;
                return launch_tail<kern>({egrid, smem, c.stream, step ? "cs2::ad_ens_step_kernel" : "cs2::ad_ens_kernel"}, ens);
            } else {
                constexpr auto kern = STEP ? ad_step_kernel<T, REG, FIX> : ad_masked_kernel<T, REG, FIX>;
                return launch_tail<kern>({grid, smem, c.stream, step ? "cs2::ad_step_kernel" : "cs2::ad_masked_kernel"}, args);
            }
        },
        c.p->LREGCL != 0, c.p->AD_TRAJ_FIX != 0, step, nmem > 0, c.is(kShared));
}

template int launch_ad_masked<double>(const ADCall<double>&);
template int launch_ad_masked<float>(const ADCall<float>&);

// ------------------------------------------------------------------------------------------------------------------
// Masked adjoint over `ndir` DIRECTIONS on one trajectory (BUILD EXTENSION, C ABI cloudsc2_ad_multi_* /
// cloudsc2_ad_multi_step_*): a block of rows of the Jacobian (`jacrev`), several cost functionals on one trajectory.
// Direction d of a present forcing lies d * in_ds elements behind direction 0, direction d of a wanted adjoint d * out_ds
// elements.  A sibling of ad_masked_sweep (same ad_forward / ad_backward, same parking, same zero line).  Only ad_backward
// depends on the cotangent, so
//   * per column the level table, the pre-scan and crh_setup are formed once; per level the 16 (STEP: 15) state words, `aph`
//     and the two trajectory flux words are loaded once (next level prefetched), ad_forward - the nonlinear recomputation
//     with all its exponentials - runs once, and with STEP saturation_point_d runs once (its value is saturation_point's
//     bit for bit, see there);
//   * inside the level a RUNTIME loop over the directions loads one direction's nine forcing words ahead (the next
//     direction of this level, or direction 0 of the level above), calls the unchanged ad_backward on the level's ADTraj
//     and stores under `want`.  ad_backward writes nothing into the ADTraj but what ad_unpark reloads from LDS (fp32) - the
//     very words ad_park stored once in front of the direction loop - so every direction sees the single launch's words;
//   * the backward carry (ADBack without the evaporation members: six words per direction) lives in LDS slots
//     [word][d][threadIdx.x] that no other lane touches: no barrier.  The launcher sizes the slots by the call's ndir;
//   * the direction base is wave-uniform: it is added to the field pointer as a 64-bit scalar (an absent forcing keeps the
//     zero line's pointer), the per-lane offsets stay 32-bit.  Every load is issued; at the last direction of level 0 the
//     look-ahead re-reads direction 0 of that level;
//   * STORES: ad_masked_sweep holds a level's eleven results one iteration late; eleven per direction do not fit 256 VGPRs
//     beside an ADTraj that has to survive the direction loop.  A direction's results are stored in plain order, behind
//     its ad_backward, followed by drain_vmem (as tl_dirs_sweep): with the store count unknown hipcc's next wait would
//     cover them anyway, and the explicit drain sits behind a whole ad_backward, where the look-ahead words (issued in
//     front of it) have arrived.
constexpr int kADCarryWords = 6;   // tmp_rfln_i, tmp_sfln_i, rfl_i, sfl_i, daph_i, dp_i

template <typename T>
inline size_t ad_dirs_lds_bytes(int nz, int ndir) {
    return (2 * size_t(nz + 1) + (kADPark<T> ? size_t(CS2_AD_PARK_COUNT) * kColBlock : 0) +
            size_t(kADCarryWords) * ndir * kColBlock) * sizeof(T);
}

//
// The same call for every MEMBER of an ensemble (ad_mdirs_kernel / ad_mdirs_step_kernel, C ABI cloudsc2_ad_multi_ens_* /
// cloudsc2_ad_multi_step_ens_*): members times directions in one launch, an ensemble of Jacobian row blocks.  ENS on the sweep
// below, as on ad_masked_sweep: one workgroup serves one column block of one member (ens_block).  The state and the two
// trajectory fluxes of member m lie m * ms elements behind member 0 (ADMemberFields); direction d of member m of a present
// forcing lies m * in_ms + d * in_ds elements behind the call's pointer, of a wanted adjoint m * out_ms + d * out_ds (member-
// major batches; the three member strides are independent because states, cotangents and results are three allocations of
// different sizes).  All bases are wave-uniform 64-bit scalars added to the pointer; nothing else differs from the single
// form: the carry slots are per workgroup, and a workgroup sees one member only.
// Words moved per member, level and column: 16 (STEP: 15) + 2 + ndir * (present in_adj + present out_adj) - the single
// multi-direction call's; what the one launch saves over a loop over the members is nmem - 1 launches with their level
// tables and pre-scans, and the idle CUs of a small member's grid.
template <typename T, bool REG, bool FIX, bool STEP, bool ENS = false>
__device__ __forceinline__ void ad_dirs_sweep(const ADDirsArgs<T>& A, const EnsGeom g = EnsGeom{}, const int64_t in_ms = 0,
                                              const int64_t out_ms = 0) {
    Ext<T> e = A.m.e;
    NLK<T> kc = A.m.kc;
    ExpK<T> xk = A.m.xk;
    const int nx = A.m.nx, nz = A.m.nz, ndir = A.ndir;
    const int64_t ls = A.m.ls, in_ds = A.in_ds, out_ds = A.out_ds;
    const T* __restrict__ eta = A.m.eta;
    T dt = A.m.dt;
    const uint32_t have = A.m.have, want = A.m.want;
    typename std::conditional<ENS, ADMemberFields<T>, ADMaskedFields<T>>::type F;
    const auto F_in = [&](int i) { return F.in(i); };
    extern __shared__ __align__(16) unsigned char smem_raw[];
    T* s_eta = reinterpret_cast<T*>(smem_raw);
    T* s_scalm = s_eta + (nz + 1);
    int klo, khi;
    build_level_table<T>(eta, nz, e, s_eta, s_scalm, klo, khi);
    if constexpr (sizeof(T) == 8) {
        pin_vgprs(e.RCPD, e.RLSTT, e.RLVTT, e.R4LES, e.R4IES, e.RTT, e.R3IES, e.R3LES, e.R2ES, e.ZQMAX, e.RETV, e.R5LES,
                  e.R5IES, e.RG, e.RD, kc.rdt, kc.cons2, kc.rRD, kc.rRCPD, dt);
        pin_expk(xk);
    }

    int gcol;
    int64_t imb = 0, omb = 0;   // ENS: this member's base in the batched forcings / adjoints (elements; wave-uniform)
    if constexpr (ENS) {
        int member;
        gcol = ens_block(g.bpm, member) * kColBlock + threadIdx.x;
        F.mb = member * g.ms;
        imb = member * in_ms;
        omb = member * out_ms;
    } else {
        gcol = xcd_block() * kColBlock + threadIdx.x;
    }
    T* const park_lds = s_scalm + (nz + 1) + threadIdx.x;
    // word w of direction d: s_carry[(w * ndir + d) * kColBlock], behind the parking slots
    T* const s_carry = park_lds + (kADPark<T> ? CS2_AD_PARK_COUNT * kColBlock : 0);
    if (gcol >= nx) return;  // no later workgroup barrier: whole lanes may retire
    using O = uint32_t;
    const O lsb = O(ls) * O(sizeof(T));
    const O colb = O(gcol) * O(sizeof(T));
    const O zo = O(threadIdx.x & (kWave - 1)) * O(sizeof(T));   // this lane's word of the zero line
    const auto slot = [&](int w, int d) -> T& { return s_carry[(w * ndir + d) * kColBlock]; };

    const T trpaus = trpaus_prescan<T, false, O>(F.in(NL_IN_T), F.in(NL_IN_TND_CML_T), lsb, colb, dt, s_eta, klo, khi);
    const CrhCol<T> crh = crh_setup<T>(trpaus);

    for (int d = 0; d < ndir; ++d)
        for (int w = 0; w < kADCarryWords; ++w) slot(w, d) = T(0.0);

    // forcing words of direction d for the level at byte offset o
    const auto load_dir = [&](int d, O o) {
        const ADDirFields<T> Fd{F, have, imb + d * in_ds, int64_t(0)};
        return ad_load_force_masked<T>(Fd, have, lsb, o, zo);
    };
    // ONE loop, k = nz .. 0, and no batch of loads outside it (see ad_masked_sweep: hipcc lays a prologue out around the loop
    // as it pleases, and check_ring_isa.check_prefetch_distance reads every backward branch as a loop): iteration k requests
    // level k-1's state words and computes level k; the first iteration only requests - its direction loop runs the last
    // direction's look-ahead alone, which is direction 0 of level nz-1.
    O o = O(nz) * lsb + colb;
    LevelIn<T> xa = zero_level<T>();
    ADForce<T> fa = zero_force<T>();
    T aph_k = ldg(F.in(NL_IN_APH), o), sfl = T(0.0), rfl = T(0.0);   // aph[nz]: level nz-1's lower half level
    for (int k = nz; k >= 0; --k) {
        const bool more = k > 0, live = k < nz;
        LevelIn<T> xn = xa;
        T aph_n = aph_k, sfl_n = sfl, rfl_n = rfl;
        if (more) {
            const O om = o - lsb;
            xn = load_level<T>(F_in, lsb, om, STEP);
            xn.aph1 = aph_k;   // aph[k]: already here as this level's upper half level
            aph_n = ldg(F.in(NL_IN_APH), om);
            sfl_n = ldg(F.traj_n(), om);
            rfl_n = ldg(F.traj_l(), om);
        }
        T g_t = T(0.0), g_ap = T(0.0);
        ADTraj<T> r;
        if (live) {
            if constexpr (STEP) {
                const SatD<T> s = saturation_point_d<T, 0>(e, xk, xa.t, xa.ap);
                xa.qsat = s.qsat;
                g_t = s.g_t;
                g_ap = s.g_ap;
            }
            ad_forward<T, FIX, false>(e, kc, xk, xa, aph_k, k, s_eta[k], s_scalm[k], crh, dt, rfl, sfl, T(0.0), T(1.0), r);
            if constexpr (kADPark<T>) ad_park<T>(park_lds, r);
        }
        for (int d = live ? 0 : ndir - 1; d < ndir; ++d) {
            F.fresh();
            const bool last = d + 1 == ndir;
            const ADForce<T> fn = load_dir(last ? 0 : d + 1, last && more ? o - lsb : o);
            if (live) {
                ADBack<T> b;
                b.tmp_rfln_i = slot(0, d); b.tmp_sfln_i = slot(1, d); b.rfl_i = slot(2, d); b.sfl_i = slot(3, d);
                b.daph_i = slot(4, d); b.dp_i = slot(5, d);
                b.covptot_i = b.aph_s_i = T(0.0);
                b.aph_s = T(1.0);
                const ADOut<T> a = ad_backward<T, REG, FIX, false>(e, kc, xa, k, s_scalm[k], dt, sfl, r, fa, b, park_lds);
                slot(0, d) = b.tmp_rfln_i; slot(1, d) = b.tmp_sfln_i; slot(2, d) = b.rfl_i; slot(3, d) = b.sfl_i;
                slot(4, d) = b.daph_i; slot(5, d) = b.dp_i;
                const ADDirFields<T> Fd{F, have, int64_t(0), omb + d * out_ds};
                ad_store_masked<T, STEP>(Fd, want, lsb, o, dt, a, g_ap * a.qsat, g_t * a.qsat);
                drain_vmem();   // see drain_vmem
            }
            fa = fn;
        }
        xa = xn;
        aph_k = aph_n;
        sfl = sfl_n;
        rfl = rfl_n;
        o -= lsb;
    }
    // :982-986 top half level, per direction
    for (int d = 0; d < ndir; ++d) {
        const int64_t ob = omb + d * out_ds;
        if (want >> NL_IN_APH & 1u) stg(F.oadj(NL_IN_APH) + ob, colb, slot(4, d) - slot(5, d));
        if (want >> NL_IN_LU & 1u) stg(F.oadj(NL_IN_LU) + ob, colb, T(0.0));
    }
}

template <typename T, bool REG, bool FIX>
__global__ void __launch_bounds__(kColBlock)
ad_dirs_kernel(const ADDirsArgs<T> A) {
    ad_dirs_sweep<T, REG, FIX, false>(A);
}

template <typename T, bool REG, bool FIX>
__global__ void __launch_bounds__(kColBlock)
ad_dirs_step_kernel(const ADDirsArgs<T> A) {
    ad_dirs_sweep<T, REG, FIX, true>(A);
}

// ad_dirs_kernel / ad_dirs_step_kernel for the members of an ensemble, one launch (BUILD EXTENSION, C ABI
// cloudsc2_ad_multi_ens_* / cloudsc2_ad_multi_step_ens_*): see ad_dirs_sweep
template <typename T, bool REG, bool FIX>
__global__ void __launch_bounds__(kColBlock)
ad_mdirs_kernel(const ADMDirsArgs<T> A) {
    ad_dirs_sweep<T, REG, FIX, false, true>(A.d, A.g, A.in_ms, A.out_ms);
}

template <typename T, bool REG, bool FIX>
__global__ void __launch_bounds__(kColBlock)
ad_mdirs_step_kernel(const ADMDirsArgs<T> A) {
    ad_dirs_sweep<T, REG, FIX, true, true>(A.d, A.g, A.in_ms, A.out_ms);
}

// launch_ad_masked for `ndir` directions (1 <= ndir <= kADMaxDirs, checked by the caller): in_adj[f] / out_adj[f] point at
// direction 0; the strides are in elements.  kEns: the ensemble form (ad_mdirs_kernel / ad_mdirs_step_kernel) - every pointer
// is member 0's, direction 0's; the caller has checked nmem and the three member strides.
template <typename T>
int launch_ad_dirs(const ADCall<T>& c) {
    const int ndir = c.dirs.ndir;
    if (evap_on(*c.p) || !fits_u32_offsets<T>(c.nz, c.ls)) return -2;
    if (ndir < 1 || ndir > kADMaxDirs) return -1;
    const bool step = c.is(kStep);
    ADDirsArgs<T> args;
    args.m = fill_ad_masked_args<T>(c);
    args.in_ds = c.dirs.in_ds; args.out_ds = c.dirs.out_ds; args.ndir = ndir;
    const int nmem = c.is(kEns) ? c.members.nmem : 0;
    const int bpm = (c.nx + kColBlock - 1) / kColBlock;
    if (nmem > 0 && int64_t(nmem) * bpm > kMaxGrid) return -2;   // as launch_ad_masked: the launcher holds its own grid
    const dim3 grid(bpm), egrid(unsigned(nmem > 0 ? nmem : 1) * unsigned(bpm));
    const size_t smem = ad_dirs_lds_bytes<T>(c.nz, ndir);
    // device_always: this launcher has looked the device up below 64 KiB of LDS as well since it was written (as
    // launch_tl_dirs does), so a device ordinal beyond kMaxDevices is refused here (-2) where the single-direction
    // launchers still run.  Nothing in the launch needs it; kept so that no call changes its outcome.
    return with_flags(
        [&](auto REG, auto FIX, auto STEP, auto ENS) {
            if constexpr (ENS) {
                constexpr auto kern = STEP ? ad_mdirs_step_kernel<T, REG, FIX> : ad_mdirs_kernel<T, REG, FIX>;
                const ADMDirsArgs<T> ens = {args, {c.members.ms, bpm}, c.members.in_ms, c.members.out_ms};
                return launch_tail<kern>({egrid, smem, c.stream, step ? "cs2::ad_mdirs_step_kernel" : "cs2::ad_mdirs_kernel", true},
                                         ens);
            } else {
                constexpr auto kern = STEP ? ad_dirs_step_kernel<T, REG, FIX> : ad_dirs_kernel<T, REG, FIX>;
                return launch_tail<kern>({grid, smem, c.stream, step ? "cs2::ad_dirs_step_kernel" : "cs2::ad_dirs_kernel", true}, args);
            }
        },
        c.p->LREGCL != 0, c.p->AD_TRAJ_FIX != 0, step, nmem > 0);
}

template int launch_ad_dirs<double>(const ADCall<double>&);
template int launch_ad_dirs<float>(const ADCall<float>&);

}  // namespace cs2
