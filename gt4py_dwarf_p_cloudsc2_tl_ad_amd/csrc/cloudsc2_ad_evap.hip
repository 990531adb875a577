// Trajectory adjoints WITH the evaporation block (LEVAPLS2 / LDRAIN1D; BUILD EXTENSION, C ABI cloudsc2_ad_evap_*,
// cloudsc2_ad_evap_step_*, cloudsc2_ad_evap_multi_*, cloudsc2_ad_evap_multi_step_*, and for the members of an ensemble
// cloudsc2_ad_evap_ens_*, cloudsc2_ad_evap_step_ens_*).
//
// The masked, step and multi-direction adjoints of cloudsc2_ad.hip read their trajectory - the two precipitation fluxes
// entering each level - from a cloudsc2_nl / cloudsc2_tl call on the same state and have no forward sweep.  With the
// evaporation block the precipitation cover entering a level (tmp_covptotp) is a second loop-carried trajectory value, and
// no NL output holds it: out_covptot is 0 both where the block did not run and where everything evaporated under a clear
// sky.  The kernels here therefore run TWO sweeps in one launch, one lane per column:
//   sweep 1 (k = 0 .. nz-1; skipped when `cover_ready`): the level's state words and the two fluxes entering it (from the
//           trajectory fields, not carried: the level's ad_forward is then the very computation sweep 2 repeats),
//           ad_forward<T, FIX, true>, and ONE store - the cover entering level k to `cover[k]`, a caller-owned field; the
//           level's resulting cover is carried.  hipcc drops what of ad_forward the cover does not depend on;
//   sweep 2 (k = nz-1 .. 0): a copy of the loop of ad_masked_sweep (kept apart from it: docs/TUNING_LOG.md 3.23; one level
//           of prefetch, absent forcings from the zero line, stores one iteration late under `want`, fp32 parking) with EVAP = true: `cover[k]` joins the level batch, the forcing
//           on covptot is read, aph[nz] is the surface pressure, and the accumulated adjoint of the surface pressure is
//           added into out_adj[NL_IN_APH] at level nz behind the loop (ad_kernel's :970-971).
// A lane's cover words are written and later read by that lane only: no cross-lane dependency, no barrier (as with the
// dense kernel's parking in out_mfd_i).
// Words per level and column: sweep 1 reads 16 (STEP: 15) + 2 and writes 1; sweep 2 moves 16 (15) + 2 + 1 + ndir x
// (present forcings + wanted adjoints).  include/cloudsc2_hip.h has the comparison with the dense call.
#include "cloudsc2_ad_level.hpp"

namespace cs2 {

template <typename T>
struct ADCoverArgs {
    ADMaskedArgs<T> m;             // at kernarg offset 0: ADMaskedFields reads the pointers from there
    T* cover;                      // [nz+1 levels][lev_stride]: level k = the cover entering level k; level nz is not touched
    int cover_ready;               // != 0: `cover` is already filled for this state and trajectory; sweep 1 is skipped
};
// The single kernels for every MEMBER of an ensemble (ad_cover_ens_kernel / ad_cover_ens_step_kernel, C ABI
// cloudsc2_ad_evap_ens_* / cloudsc2_ad_evap_step_ens_*): ad_ens_kernel's member decode (ens_block) and base add (ADEnsFields),
// and `cover` is batched like every other field - the member's base is added to it as well.
template <typename T>
struct ADCoverEnsArgs {
    ADCoverArgs<T> c;              // at kernarg offset 0 (its ADMaskedArgs first: ADEnsFields reads the pointers from there)
    EnsGeom g;
};
template <typename T>
struct ADCoverDirsArgs {
    ADDirsArgs<T> d;               // at kernarg offset 0 (its ADMaskedArgs first)
    T* cover;
    int cover_ready;
};

// The backward carry of one direction in LDS: tmp_rfln_i + rfl_i, tmp_sfln_i + sfl_i, daph_i, dp_i, covptot_i, aph_s_i.
// ad_backward only ever reads the first two pairs as sums, and leaves one word of each pair zero (a level that melts
// moves tmp_*_i into *fl_i, a level that does not sets *fl_i = 0): the sums are exact, the adjoints the single kernel's.
constexpr int kADCoverCarryWords = 6;
// Values of CS2_AD_PARK_LIST the multi-direction kernels park.  fp32: all, as everywhere.  fp64: the level's ADTraj has to
// survive the direction loop, and with the evaporation block's 21 words it no longer fits 256 VGPRs + 256 AGPRs beside the
// prefetched next level (116 - 172 bytes of scratch per lane unparked); a parked value is reloaded by every direction's
// ad_backward and is dead across the loop.  CS2_AD_DIRS_PARK64 of them fit the 160 KB beside eight directions' carries.
#ifndef CS2_AD_DIRS_PARK64
#define CS2_AD_DIRS_PARK64 16
#endif
template <typename T>
constexpr int kADCoverDirsPark = sizeof(T) == 4 ? CS2_AD_PARK_COUNT : CS2_AD_DIRS_PARK64;
// fp64 only, the other half: words of the evaporation block that ad_backward reads in its FIRST half only.  Unparked they
// stay live through the second half of every direction for the next one's sake; reloaded in front of each direction's
// ad_backward they are dead from their last use on.  Same slot layout and the same fences as ad_park / ad_unpark.
#define CS2_AD_EVAP_PARK_LIST(X) \
    X(prtot) X(rfln2) X(sfln2) X(corqs) X(qlim) X(preclr1) X(romc) X(qe) X(sq) X(xx) X(beta) X(rtmp1) X(b) X(dpr)
#define CS2_AD_EVAP_PARK_COUNT 14
template <typename T>
constexpr int kADCoverDirsParkEvap = sizeof(T) == 4 ? 0 : CS2_AD_EVAP_PARK_COUNT;
template <typename T>
__device__ __forceinline__ void ad_park_evap(T* __restrict__ lds, const ADTraj<T>& r) {
    int j = 0;
#define CS2_X(f) lds[(j++) * kColBlock] = r.f;
    CS2_AD_EVAP_PARK_LIST(CS2_X)
#undef CS2_X
    asm volatile("" ::: "memory");
}
template <typename T>
__device__ __forceinline__ void ad_unpark_evap(const T* __restrict__ lds, ADTraj<T>& r) {
    asm volatile("" ::: "memory");
    int j = 0;
#define CS2_X(f) r.f = lds[(j++) * kColBlock];
    CS2_AD_EVAP_PARK_LIST(CS2_X)
#undef CS2_X
}

template <typename T>
inline size_t ad_cover_dirs_lds_bytes(int nz, int ndir) {
    return (2 * size_t(nz + 1) + size_t(kADCoverDirsPark<T> + kADCoverDirsParkEvap<T>) * kColBlock +
            size_t(kADCoverCarryWords) * ndir * kColBlock) * sizeof(T);
}

// What both sweeps of a column need, set up once: constants, level table, this lane's offsets, the critical relative humidity
// profile and the surface pressure.
template <typename T>
struct ADCoverCol {
    Ext<T> e;
    NLK<T> kc;
    ExpK<T> xk;
    T dt;
    int nz;
    uint32_t lsb, colb, zo;
    T* s_eta;
    T* s_scalm;
    T* park_lds;
    CrhCol<T> crh;
    T aph_s, aph_top;              // aph[nz] (:146 the surface pressure), aph[0]
};

// -> false: this lane has no column (it retires; there is no later workgroup barrier).  ENS: one member of an ensemble per
// workgroup (`g`: EnsGeom; `F`: ADEnsFields, whose member base is set here)
template <typename T, bool ENS = false, typename FP>
__device__ __forceinline__ bool ad_cover_setup(const ADMaskedArgs<T>& A, FP& F, ADCoverCol<T>& c, const EnsGeom g = EnsGeom{}) {
    c.e = A.e;
    c.kc = A.kc;
    c.xk = A.xk;
    c.nz = A.nz;
    c.dt = A.dt;
    const int nx = A.nx, nz = A.nz;
    const int64_t ls = A.ls;
    const T* __restrict__ eta = A.eta;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    c.s_eta = reinterpret_cast<T*>(smem_raw);
    c.s_scalm = c.s_eta + (nz + 1);
    int klo, khi;
    build_level_table<T>(eta, nz, c.e, c.s_eta, c.s_scalm, klo, khi);
    // No pin_vgprs / pin_expk here (ad_masked_sweep pins 20 fp64 constants and the exponential's coefficients in VGPRs): with
    // the evaporation block's trajectory words live as well, the pinned fp64 instantiations spill (12 - 28 bytes of scratch
    // in the single kernels, ~420 in the multi-direction ones); unpinned, the single kernels need 256 + ~190 registers.
    int gcol;
    if constexpr (ENS) {
        int member;
        gcol = ens_block(g.bpm, member) * kColBlock + threadIdx.x;
        F.mb = member * g.ms;
        F.have = A.have;
    } else {
        gcol = xcd_block() * kColBlock + threadIdx.x;
    }
    c.park_lds = c.s_scalm + (nz + 1) + threadIdx.x;
    if (gcol >= nx) return false;
    c.lsb = uint32_t(ls) * uint32_t(sizeof(T));
    c.colb = uint32_t(gcol) * uint32_t(sizeof(T));
    c.zo = uint32_t(threadIdx.x & (kWave - 1)) * uint32_t(sizeof(T));   // this lane's word of the zero line
    c.aph_s = ldg(F.in(NL_IN_APH), uint32_t(nz) * c.lsb + c.colb);      // :146 surface pressure
    c.aph_top = ldg(F.in(NL_IN_APH), c.colb);
    const T trpaus = trpaus_prescan<T, false, uint32_t>(F.in(NL_IN_T), F.in(NL_IN_TND_CML_T), c.lsb, c.colb, c.dt, c.s_eta,
                                                        klo, khi);
    c.crh = crh_setup<T>(trpaus);
    landed(c.aph_top);
    landed(c.aph_s);   // loaded in front of the level loops, first read inside them (see landed)
    return true;
}

// Sweep 1: cover[k] = the precipitation cover entering level k, k = 0 .. nz-1.
template <typename T, bool FIX, bool STEP, typename FP>
__device__ __forceinline__ void ad_cover_fill(FP& F, const ADCoverCol<T>& c, T* __restrict__ cover) {
    using O = uint32_t;
    const auto F_in = [&](int i) { return F.in(i); };
    const int nz = c.nz;
    const O lsb = c.lsb;
    // ONE loop, k = -1 .. nz-1, and no batch of loads outside it (see ad_masked_sweep): iteration k requests level k+1's
    // words and computes level k; the first iteration only requests
    O o = c.colb - lsb;   // level -1: only o + lsb is formed from it
    T covptot = T(0.0);
    T aph_k = c.aph_top;
    LevelIn<T> xa = zero_level<T>();
    T sfl = T(0.0), rfl = T(0.0);
    // (not peeled: hipcc otherwise takes the first, load-only iteration out of this short loop as a prologue batch)
#pragma clang loop unroll(disable)
    for (int k = -1; k < nz; ++k) {
        F.fresh();
        LevelIn<T> xn = xa;
        T sfl_n = sfl, rfl_n = rfl;
        if (k + 1 < nz) {
            xn = load_level<T>(F_in, lsb, o + lsb, STEP);
            sfl_n = ldg(F.traj_n(), o + lsb);
            rfl_n = ldg(F.traj_l(), o + lsb);
        }
        if (k >= 0) {
            if constexpr (STEP) xa.qsat = saturation_point<T, 0>(c.e, c.xk, xa.t, xa.ap);
            ADTraj<T> r;
            ad_forward<T, FIX, true>(c.e, c.kc, c.xk, xa, aph_k, k, c.s_eta[k], c.s_scalm[k], c.crh, c.dt, rfl, sfl, covptot,
                                     c.aph_s, r);
            stg(cover, o, covptot);
            covptot = r.covptot;
            aph_k = xa.aph1;
        }
        xa = xn;
        sfl = sfl_n;
        rfl = rfl_n;
        o += lsb;
    }
}

// ad_load_force_masked + the forcing on covptot, which only the evaporation block reads (raw, as the other nine words)
template <typename T, typename FP>
__device__ __forceinline__ ADForce<T> ad_cover_load_force(const FP& F, uint32_t have, uint32_t lsb, uint32_t o, uint32_t zo) {
    ADForce<T> f = ad_load_force_masked<T>(F, have, lsb, o, zo);
    f.covptot = ldg(F.adj(NL_OUT_COVPTOT), (have >> NL_OUT_COVPTOT & 1u) ? o : zo);
    return f;
}

// Single direction: ad_masked_sweep's loop with the evaporation block (see the head of this file and ad_masked_sweep).
// ENS: one member of an ensemble per workgroup; the member's base is added to `cover` as to every field pointer.  Every
// pointer then costs a second SGPR pair (the sum), and with the pointers of a whole level batch fetched at once
// ad_cover_ens_kernel<double, true, true> computed wrong adjoints on an MI355X in the columns where the evaporation block
// runs (fp32 and the step form of the same text gave the single kernel's bits).  NOT explained: docs/TUNING_LOG.md 3.25 lists
// what was ruled out.  With `fresh()` between the batches of a level - state, forcing, the rest, the stores - the kernarg
// loads stay beside their uses and all sixteen instantiations give the single kernels' results.  That is held by tests
// alone (tests/test_hip_evap_ensemble.py: every instantiation, and the fp64 kernels on a full chip against the looped
// launches): rerun them after any change to this sweep, to ADEnsFields or to the compiler.
template <typename T, bool REG, bool FIX, bool STEP, bool ENS = false>
__device__ __forceinline__ void ad_cover_sweep(const ADCoverArgs<T>& A, const EnsGeom g = EnsGeom{}) {
    typename std::conditional<ENS, ADEnsFields<T>, ADMaskedFields<T>>::type F;
    ADCoverCol<T> c;
    if (!ad_cover_setup<T, ENS>(A.m, F, c, g)) return;
    const auto F_in = [&](int i) { return F.in(i); };
    const uint32_t have = A.m.have, want = A.m.want;
    T* __restrict__ cover = A.cover;
    if constexpr (ENS) cover += F.mb;
    if (A.cover_ready == 0) ad_cover_fill<T, FIX, STEP>(F, c, cover);

    using O = uint32_t;
    const int nz = c.nz;
    const O lsb = c.lsb, colb = c.colb, zo = c.zo;
    const T dt = c.dt;
    ADBack<T> b = zero_back<T>(c.aph_s);
    // ONE loop, k = nz .. -1: iteration k requests level k-1's words, stores level k+1's adjoints and computes level k
    O o = O(nz) * lsb + colb, po = o;
    ADOut<T> pa = zero_out<T>();
    LevelIn<T> xa = zero_level<T>();
    ADForce<T> fa = zero_force<T>();
    T aph_k = c.aph_s, sfl = T(0.0), rfl = T(0.0), cov = T(0.0);   // aph[nz]: level nz-1's lower half level
    T pt = T(273.0), pap = T(1.0e5);   // STEP: t and ap of the level whose adjoints `pa` holds
    for (int k = nz; k >= -1; --k) {
        F.fresh();
        LevelIn<T> xn = xa;
        ADForce<T> fn = fa;
        T aph_n = aph_k, sfl_n = sfl, rfl_n = rfl, cov_n = cov;
        if (k > 0) {
            const O om = o - lsb;
            xn = load_level<T>(F_in, lsb, om, STEP);
            xn.aph1 = aph_k;   // aph[k]: already here as this level's upper half level
            if constexpr (ENS) F.fresh();   // see the head of this function
            fn = ad_cover_load_force<T>(F, have, lsb, om, zo);
            if constexpr (ENS) F.fresh();
            aph_n = ldg(F.in(NL_IN_APH), om);
            sfl_n = ldg(F.traj_n(), om);
            rfl_n = ldg(F.traj_l(), om);
            cov_n = ldg(static_cast<const T*>(cover), om);
        }
        if constexpr (ENS) F.fresh();
        if (k < nz - 1) {
            if constexpr (STEP) {
                const SatD<T> s = saturation_point_d<T, 0>(c.e, c.xk, pt, pap);
                ad_store_masked<T, true>(F, want, lsb, po, dt, pa, s.g_ap * pa.qsat, s.g_t * pa.qsat);
            } else {
                ad_store_masked<T>(F, want, lsb, po, dt, pa);
            }
        }
        if (k >= 0 && k < nz) {
            if constexpr (STEP) xa.qsat = saturation_point<T, 0>(c.e, c.xk, xa.t, xa.ap);
            ADTraj<T> r;
            ad_forward<T, FIX, true>(c.e, c.kc, c.xk, xa, aph_k, k, c.s_eta[k], c.s_scalm[k], c.crh, dt, rfl, sfl, cov,
                                     c.aph_s, r);
            if constexpr (kADPark<T>) ad_park<T>(c.park_lds, r);
            pa = ad_backward<T, REG, FIX, true>(c.e, c.kc, xa, k, c.s_scalm[k], dt, sfl, r, fa, b, c.park_lds);
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
        cov = cov_n;
        o -= lsb;
    }
    if (want >> NL_IN_APH & 1u) {
        // :970-971: out_aph_i[nz] (stored by level nz-1 above) also receives the accumulated tmp_aph_s_i
        const O on = O(nz) * lsb + colb;
        T* const oaph = F.oadj(NL_IN_APH);
        stg(oaph, on, ldg(static_cast<const T*>(oaph), on) + b.aph_s_i);
        stg(oaph, colb, b.daph_i - b.dp_i);   // :982-986 top half level
    }
    if (want >> NL_IN_LU & 1u) stg(F.oadj(NL_IN_LU), colb, T(0.0));
}

template <typename T, bool REG, bool FIX>
__global__ void __launch_bounds__(kColBlock, sizeof(T) == 4 ? 2 : 1)
ad_cover_kernel(const ADCoverArgs<T> A) {
    ad_cover_sweep<T, REG, FIX, false>(A);
}

template <typename T, bool REG, bool FIX>
__global__ void __launch_bounds__(kColBlock, sizeof(T) == 4 ? 2 : 1)
ad_cover_step_kernel(const ADCoverArgs<T> A) {
    ad_cover_sweep<T, REG, FIX, true>(A);
}

// ad_cover_kernel / ad_cover_step_kernel for the members of an ensemble, one launch: see ADCoverEnsArgs
template <typename T, bool REG, bool FIX>
__global__ void __launch_bounds__(kColBlock, sizeof(T) == 4 ? 2 : 1)
ad_cover_ens_kernel(const ADCoverEnsArgs<T> A) {
    ad_cover_sweep<T, REG, FIX, false, true>(A.c, A.g);
}

template <typename T, bool REG, bool FIX>
__global__ void __launch_bounds__(kColBlock, sizeof(T) == 4 ? 2 : 1)
ad_cover_ens_step_kernel(const ADCoverEnsArgs<T> A) {
    ad_cover_sweep<T, REG, FIX, true, true>(A.c, A.g);
}

// `ndir` directions on one trajectory: ad_dirs_sweep with the evaporation block.  Sweep 1 runs once; per level ad_forward
// runs once and ad_backward per direction; the per-direction backward carry in LDS is six words (kADCoverCarryWords).
template <typename T, bool REG, bool FIX, bool STEP>
__device__ __forceinline__ void ad_cover_dirs_sweep(const ADCoverDirsArgs<T>& A) {
    ADMaskedFields<T> F;
    ADCoverCol<T> c;
    const int ndir = A.d.ndir;
    const int64_t in_ds = A.d.in_ds, out_ds = A.d.out_ds;
    if (!ad_cover_setup<T>(A.d.m, F, c)) return;
    const auto F_in = [&](int i) { return F.in(i); };
    const uint32_t have = A.d.m.have, want = A.d.m.want;
    T* __restrict__ cover = A.cover;
    if (A.cover_ready == 0) ad_cover_fill<T, FIX, STEP>(F, c, cover);

    using O = uint32_t;
    const int nz = c.nz;
    const O lsb = c.lsb, colb = c.colb, zo = c.zo;
    const T dt = c.dt;
    // word w of direction d: s_carry[(w * ndir + d) * kColBlock], behind the parking slots
    constexpr int PARK = kADCoverDirsPark<T>;
    constexpr int PARK_EVAP = kADCoverDirsParkEvap<T>;
    T* const park_evap = c.park_lds + PARK * kColBlock;
    T* const s_carry = park_evap + PARK_EVAP * kColBlock;
    const auto slot = [&](int w, int d) -> T& { return s_carry[(w * ndir + d) * kColBlock]; };
    for (int d = 0; d < ndir; ++d)
        for (int w = 0; w < kADCoverCarryWords; ++w) slot(w, d) = T(0.0);
    const auto load_dir = [&](int d, O o) {
        const ADDirFields<T> Fd{F, have, d * in_ds, int64_t(0)};
        return ad_cover_load_force<T>(Fd, have, lsb, o, zo);
    };
    // ONE loop, k = nz .. 0 (see ad_dirs_sweep): iteration k requests level k-1's state words and computes level k; the
    // first iteration only requests - its direction loop runs the last direction's look-ahead alone
    O o = O(nz) * lsb + colb;
    LevelIn<T> xa = zero_level<T>();
    ADForce<T> fa = zero_force<T>();
    T aph_k = c.aph_s, sfl = T(0.0), rfl = T(0.0), cov = T(0.0);
    for (int k = nz; k >= 0; --k) {
        const bool more = k > 0, live = k < nz;
        LevelIn<T> xn = xa;
        T aph_n = aph_k, sfl_n = sfl, rfl_n = rfl, cov_n = cov;
        if (more) {
            const O om = o - lsb;
            xn = load_level<T>(F_in, lsb, om, STEP);
            xn.aph1 = aph_k;
            aph_n = ldg(F.in(NL_IN_APH), om);
            sfl_n = ldg(F.traj_n(), om);
            rfl_n = ldg(F.traj_l(), om);
            cov_n = ldg(static_cast<const T*>(cover), om);
        }
        T g_t = T(0.0), g_ap = T(0.0);
        ADTraj<T> r;
        if (live) {
            if constexpr (STEP) {
                const SatD<T> s = saturation_point_d<T, 0>(c.e, c.xk, xa.t, xa.ap);
                xa.qsat = s.qsat;
                g_t = s.g_t;
                g_ap = s.g_ap;
            }
            ad_forward<T, FIX, true>(c.e, c.kc, c.xk, xa, aph_k, k, c.s_eta[k], c.s_scalm[k], c.crh, dt, rfl, sfl, cov,
                                     c.aph_s, r);
            ad_park<T, PARK>(c.park_lds, r);
            if constexpr (PARK_EVAP > 0) ad_park_evap<T>(park_evap, r);
        }
        for (int d = live ? 0 : ndir - 1; d < ndir; ++d) {
            F.fresh();
            const bool last = d + 1 == ndir;
            const ADForce<T> fn = load_dir(last ? 0 : d + 1, last && more ? o - lsb : o);
            if (live) {
                ADBack<T> b;
                b.tmp_rfln_i = slot(0, d); b.tmp_sfln_i = slot(1, d); b.rfl_i = b.sfl_i = T(0.0);
                b.daph_i = slot(2, d); b.dp_i = slot(3, d); b.covptot_i = slot(4, d); b.aph_s_i = slot(5, d);
                b.aph_s = c.aph_s;
                if constexpr (PARK_EVAP > 0) ad_unpark_evap<T>(park_evap, r);
                const ADOut<T> a = ad_backward<T, REG, FIX, true, PARK>(c.e, c.kc, xa, k, c.s_scalm[k], dt, sfl, r, fa, b,
                                                                        c.park_lds);
                slot(0, d) = b.tmp_rfln_i + b.rfl_i; slot(1, d) = b.tmp_sfln_i + b.sfl_i;
                slot(2, d) = b.daph_i; slot(3, d) = b.dp_i; slot(4, d) = b.covptot_i; slot(5, d) = b.aph_s_i;
                const ADDirFields<T> Fd{F, have, int64_t(0), d * out_ds};
                ad_store_masked<T, STEP>(Fd, want, lsb, o, dt, a, g_ap * a.qsat, g_t * a.qsat);
                drain_vmem();   // see drain_vmem
            }
            fa = fn;
        }
        xa = xn;
        aph_k = aph_n;
        sfl = sfl_n;
        rfl = rfl_n;
        cov = cov_n;
        o -= lsb;
    }
    // per direction: :970-971 the surface half level, :982-986 the top half level
    for (int d = 0; d < ndir; ++d) {
        const int64_t ob = d * out_ds;
        if (want >> NL_IN_APH & 1u) {
            const O on = O(nz) * lsb + colb;
            T* const oaph = F.oadj(NL_IN_APH) + ob;
            stg(oaph, on, ldg(static_cast<const T*>(oaph), on) + slot(5, d));
            stg(oaph, colb, slot(2, d) - slot(3, d));
        }
        if (want >> NL_IN_LU & 1u) stg(F.oadj(NL_IN_LU) + ob, colb, T(0.0));
    }
}

template <typename T, bool REG, bool FIX>
__global__ void __launch_bounds__(kColBlock)
ad_cover_dirs_kernel(const ADCoverDirsArgs<T> A) {
    ad_cover_dirs_sweep<T, REG, FIX, false>(A);
}

template <typename T, bool REG, bool FIX>
__global__ void __launch_bounds__(kColBlock)
ad_cover_dirs_step_kernel(const ADCoverDirsArgs<T> A) {
    ad_cover_dirs_sweep<T, REG, FIX, true>(A);
}

// The caller (cloudsc2_capi.hip) has checked every argument: one of the evaporation switches is on, fields below 4 GiB,
// `cover` not NULL, and under kMulti the direction arguments (the multi-direction kernels; without it the single ones).
// kStep: in[NL_IN_QSAT] is not read, out_adj[NL_IN_QSAT] is NULL.  kEns (without kMulti only): the ensemble form of the
// single kernels - every field pointer, `cover` included, is member 0's, member m lies m * ms elements behind it; the caller
// has checked nmem and ms.
template <typename T>
int launch_ad_cover(const ADCall<T>& c) {
    const bool step = c.is(kStep);
    const int ndir = c.is(kMulti) ? c.dirs.ndir : 0, nmem = c.is(kEns) ? c.members.nmem : 0;
    if (!evap_on(*c.p) || !fits_u32_offsets<T>(c.nz, c.ls) || !c.cover.cover) return -2;
    if (ndir < 0 || ndir > kADMaxDirs || (ndir > 0 && nmem > 0)) return -1;
    ADCoverDirsArgs<T> dargs;
    ADCoverEnsArgs<T> eargs;
    ADCoverArgs<T>& sargs = eargs.c;
    (ndir > 0 ? dargs.d.m : sargs.m) = fill_ad_masked_args<T>(c);
    dargs.d.in_ds = c.dirs.in_ds; dargs.d.out_ds = c.dirs.out_ds; dargs.d.ndir = ndir;
    dargs.cover = sargs.cover = c.cover.cover;
    dargs.cover_ready = sargs.cover_ready = c.cover.cover_ready != 0;
    const int bpm = (c.nx + kColBlock - 1) / kColBlock;
    if (nmem > 0 && int64_t(nmem) * bpm > kMaxGrid) return -2;
    eargs.g.ms = c.members.ms; eargs.g.bpm = bpm;
    const dim3 grid(unsigned(nmem > 0 ? nmem : 1) * unsigned(bpm));
    const size_t smem = ndir > 0 ? ad_cover_dirs_lds_bytes<T>(c.nz, ndir)
                                 : 2 * size_t(c.nz + 1) * sizeof(T) + (kADPark<T> ? size_t(CS2_AD_PARK_COUNT) * kColBlock * sizeof(T) : 0);
    return with_flags(
        [&](auto REG, auto FIX, auto STEP, auto DIRS, auto ENS) {
            if constexpr (DIRS && ENS) {
                return -1;   // refused above: no such instantiation
            } else if constexpr (ENS) {
                constexpr auto kern = STEP ? ad_cover_ens_step_kernel<T, REG, FIX> : ad_cover_ens_kernel<T, REG, FIX>;
                return launch_tail<kern>({grid, smem, c.stream, step ? "cs2::ad_cover_ens_step_kernel" : "cs2::ad_cover_ens_kernel"},
                                         eargs);
            } else if constexpr (DIRS) {
                constexpr auto kern = STEP ? ad_cover_dirs_step_kernel<T, REG, FIX> : ad_cover_dirs_kernel<T, REG, FIX>;
                return launch_tail<kern>({grid, smem, c.stream, step ? "cs2::ad_cover_dirs_step_kernel" : "cs2::ad_cover_dirs_kernel"},
                                         dargs);
            } else {
                constexpr auto kern = STEP ? ad_cover_step_kernel<T, REG, FIX> : ad_cover_kernel<T, REG, FIX>;
                return launch_tail<kern>({grid, smem, c.stream, step ? "cs2::ad_cover_step_kernel" : "cs2::ad_cover_kernel"}, sargs);
            }
        },
        c.p->LREGCL != 0, c.p->AD_TRAJ_FIX != 0, step, ndir > 0, nmem > 0);
}

template int launch_ad_cover<double>(const ADCall<double>&);
template int launch_ad_cover<float>(const ADCall<float>&);

}  // namespace cs2
