// extern "C" boundary of libcloudsc2_hip.so - see include/cloudsc2_hip.h for the contract.
// Argument checking happens here (on the host, before anything is launched): a kernel is only
// launched when the shapes it assumes hold, because a faulting kernel can take the whole node down.
#include <cstdarg>
#include <cstdio>

#include "cloudsc2_launch.hpp"

namespace {

thread_local char g_err[512] = "";
// process-wide, not thread-local: torch.autograd runs a backward on a thread of its own, and the caller asks from another.
// The names are string literals, so a reader sees a whole name, the last one stored.
std::atomic<const char*> g_kernel{""};

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

constexpr int kMaxLevels = 4095;  // LDS table of the register-path kernels: 2 * (nz+1) * 8 B <= 64 KiB (no opt-in needed)

int check_common(const char* fn, const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls) {
    if (!p) return fail(CLOUDSC2_E_ARG, "%s: params is NULL", fn);
    if (nx < 0) return fail(CLOUDSC2_E_ARG, "%s: nx=%d < 0", fn, nx);
    if (nz < 2 || nz > kMaxLevels) return fail(CLOUDSC2_E_ARG, "%s: nz=%d outside [2, %d]", fn, nz, kMaxLevels);
    if (ls < nx) return fail(CLOUDSC2_E_ARG, "%s: lev_stride=%lld < nx=%d", fn, (long long)ls, nx);
    return 0;
}

template <typename T>
int check_ptrs(const char* fn, const char* what, const T* const* arr, int n) {
    if (!arr) return fail(CLOUDSC2_E_ARG, "%s: %s is NULL", fn, what);
    for (int i = 0; i < n; ++i)
        if (!arr[i]) return fail(CLOUDSC2_E_ARG, "%s: %s[%d] is NULL", fn, what, i);
    return 0;
}

int launched(const char* fn, int rc) {
    if (rc == 0) return CLOUDSC2_OK;
    if (rc == -2)   // the launchers' refusals: a fused build extension on fields of 4 GiB or more, or a device ordinal >= 64
        return fail(CLOUDSC2_E_UNSUPPORTED,
                    "%s: this build extension keeps 32-bit byte offsets: (nz+1) * lev_stride * sizeof(element) must be < 2^32 "
                    "bytes per field (the plain stencils cloudsc2_nl / _tl / _ad have no such limit: use them, or narrower "
                    "allocations) (or: HIP device ordinal >= 64, LDS demand beyond one CU)", fn);
    return fail(CLOUDSC2_E_LAUNCH, "%s: HIP launch failed: %s", fn, hipGetErrorString(hipPeekAtLastError()));
}

// The member arguments of the cloudsc2_*_ens_* entries (include/cloudsc2_hip.h "ENSEMBLES"); `ens` false: not such an entry.
// The bound of ONE member's extent (32-bit byte offsets) is check_masked_size's, the same as for a single masked call.
template <typename T>
int check_masked_size(const char* fn, int32_t nz, int64_t ls);
template <typename T>
int check_members(const char* fn, bool ens, int32_t nx, int32_t nz, int64_t ls, int32_t nmem, int64_t ms) {
    if (!ens) return 0;
    if (nmem < 1) return fail(CLOUDSC2_E_ARG, "%s: nmem=%d must be >= 1", fn, nmem);
    const int64_t field = int64_t(nz + 1) * ls;
    if (ms < field)
        return fail(CLOUDSC2_E_ARG, "%s: member_stride=%lld < (nz+1) * lev_stride = %lld: the members of a field would "
                    "overlap", fn, (long long)ms, (long long)field);
    if (int rc = check_masked_size<T>(fn, nz, ls)) return rc;
    const int64_t blocks = int64_t(nmem) * ((int64_t(nx) + cs2::kColBlock - 1) / cs2::kColBlock);
    if (blocks > cs2::kMaxGrid)
        return fail(CLOUDSC2_E_UNSUPPORTED, "%s: nmem * ceil(nx / %d) = %lld workgroups exceed the grid limit %lld: split "
                    "the ensemble", fn, cs2::kColBlock, (long long)blocks, (long long)cs2::kMaxGrid);
    return 0;
}

// Overlap of batched fields, judged on bounding ranges (check_shared: a written field against a shared input;
// check_cover_disjoint: the evaporation ensemble entries' `cover`): one member of a field spans
// `ea` / `eb` bytes, member m starts m * `sb` bytes behind member 0; `a` has `na` members, `b` has `nb` (1: the zero line, eta,
// a shared input).  Member i of `a` meets member j of `b` iff -ea < (a - b) + (i - j) * sb < eb.
bool member_ranges_overlap(const void* a, int64_t ea, int64_t na, const void* b, int64_t eb, int64_t nb, int64_t sb) {
    const int64_t delta = int64_t(reinterpret_cast<intptr_t>(a) - reinterpret_cast<intptr_t>(b));
    const auto floor_div = [](int64_t x, int64_t y) { return x / y - ((x % y != 0 && x < 0) ? 1 : 0); };   // y > 0
    const int64_t dmin = floor_div(-ea - delta, sb) + 1;       // the d = i - j with -ea < delta + d * sb ...
    const int64_t dmax = -floor_div(delta - eb, sb) - 1;       // ... and delta + d * sb < eb
    return std::max(dmin, -(nb - 1)) <= std::min(dmax, na - 1);
}

// The two further member arguments of the cloudsc2_*_enss_* entries (include/cloudsc2_hip.h "ENSEMBLES THAT SHARE PART OF THEIR
// STATE"; check_members has passed).  `in`: the state inputs.  `written` calls its argument with (array name, index,
// pointer) of every field the call writes; NULL pointers are skipped.  A shared input has ONE range, member 0's; a written
// field has nmem.
template <typename T, typename W>
int check_shared(const char* fn, const cs2::CallMembers& m, int32_t nx, int32_t nz, int64_t ls, const T* const* in,
                 const T* eta, const W& written) {
    const int64_t known = int64_t(0xFFFF) | CLOUDSC2_ENSS_COLUMN_MAJOR | CLOUDSC2_ENSS_MEMBER_MAJOR;
    if (m.shared_mask & ~known) {
        int bit = 0;
        while (!((uint64_t(m.shared_mask & ~known) >> bit) & 1u)) ++bit;
        return fail(CLOUDSC2_E_ARG, "%s: shared_mask bit %d is set: beyond the %d state inputs (bits 0 .. %d) and the two "
                    "block-order bits", fn, bit, NL_NUM_IN, NL_NUM_IN - 1);
    }
    if ((m.shared_mask & CLOUDSC2_ENSS_COLUMN_MAJOR) && (m.shared_mask & CLOUDSC2_ENSS_MEMBER_MAJOR))
        return fail(CLOUDSC2_E_ARG, "%s: shared_mask asks for both block orders (CLOUDSC2_ENSS_COLUMN_MAJOR and _MEMBER_MAJOR)", fn);
    if (m.eta_ms != 0 && m.eta_ms < int64_t(nz) + 1)
        return fail(CLOUDSC2_E_ARG, "%s: eta_member_stride=%lld must be 0 (one eta for all members) or >= nz + 1 = %d: the "
                    "members' level vectors would overlap", fn, (long long)m.eta_ms, nz + 1);
    if (nx == 0) return 0;
    const int64_t ext = (int64_t(nz) * ls + nx) * int64_t(sizeof(T)), sb = m.ms * int64_t(sizeof(T));
    for (int i = 0; i < NL_NUM_IN; ++i) {
        if (!(m.shared_mask >> i & 1)) continue;
        if (!in || !in[i])
            return fail(CLOUDSC2_E_ARG, "%s: shared_mask bit %d is set but in[%d] is NULL: an absent field cannot be shared", fn,
                        i, i);
        const char* what = nullptr;
        int at = 0;
        written([&](const char* name, int j, const T* f) {
            if (!what && f && member_ranges_overlap(f, ext, m.nmem, in[i], ext, 1, sb)) {
                what = name;
                at = j;
            }
        });
        if (what)
            return fail(CLOUDSC2_E_ARG, "%s: %s[%d] overlaps the shared input in[%d] in some member: every member reads a "
                        "shared input for the whole launch, no written field may share storage with it", fn, what, at, i);
    }
    if (eta && m.eta_ms != 0) {     // the members' level vectors, first to last, as ONE range: read for the whole launch too
        const int64_t rows = ((int64_t(m.nmem) - 1) * m.eta_ms + nz + 1) * int64_t(sizeof(T));
        const char* what = nullptr;
        int at = 0;
        written([&](const char* name, int j, const T* f) {
            if (!what && f && member_ranges_overlap(f, ext, m.nmem, eta, rows, 1, sb)) {
                what = name;
                at = j;
            }
        });
        if (what)
            return fail(CLOUDSC2_E_ARG, "%s: %s[%d] overlaps eta (the %d members' level vectors, eta_member_stride=%lld) in some "
                        "member: no written field may share storage with them", fn, what, at, m.nmem, (long long)m.eta_ms);
    }
    return 0;
}

// `ens`: the cloudsc2_nl_ens_* entry (nl_ens_kernel); `shared` too: cloudsc2_nl_enss_* (the same kernel on EnssGeom)
template <typename T>
int nl_impl(const char* fn, const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const T* const* in,
            const T* eta, T* const* out, double dt, void* stream, bool ens = false, const cs2::CallMembers& m = {},
            bool shared = false) {
    if (int rc = check_common(fn, p, nx, nz, ls)) return rc;
    if (int rc = check_members<T>(fn, ens, nx, nz, ls, m.nmem, m.ms)) return rc;
    if (shared)
        if (int rc = check_shared<T>(fn, m, nx, nz, ls, in, eta, [&](auto&& hit) {
                for (int i = 0; out && i < NL_NUM_OUT; ++i) hit("out", i, out[i]);
            }))
            return rc;
    if (nx == 0) return CLOUDSC2_OK;   // empty call: nothing to check or launch (zero-size tensors carry NULL pointers)
    if (int rc = check_ptrs(fn, "in", in, NL_NUM_IN)) return rc;
    if (int rc = check_ptrs(fn, "out", const_cast<const T* const*>(out), NL_NUM_OUT)) return rc;
    if (!eta) return fail(CLOUDSC2_E_ARG, "%s: eta is NULL", fn);
    if (p->ICALL != 0) return fail(CLOUDSC2_E_UNSUPPORTED, "%s: ICALL=%d (the reference implements ICALL == 0 only)", fn, p->ICALL);
    if (!(dt > 0.0)) return fail(CLOUDSC2_E_ARG, "%s: dt=%g must be > 0", fn, dt);
    if (ens)
        return launched(fn, cs2::launch_nl_ens<T>(*p, nx, nz, ls, in, eta, out, dt, static_cast<hipStream_t>(stream), nullptr,
                                                  m, shared));
    return launched(fn, cs2::launch_nl<T>(*p, nx, nz, ls, in, eta, out, dt, static_cast<hipStream_t>(stream), nullptr,
                                          0.0, nullptr, nullptr));
}

// Fused variants of cloudsc2_nl (build extensions): exactly one of `qsat_out` / `in_i` is non-NULL.  `ens`: the
// cloudsc2_nl_fused_ens_* entry (nl_ens_kernel), the saturation-fused form only.
template <typename T>
int nl_fused_impl(const char* fn, const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const T* const* in,
                  const T* const* in_i, double pf, T* qsat_out, const T* eta, T* const* out, double dt, void* stream,
                  bool ens = false, const cs2::CallMembers& m = {}, bool shared = false) {
    if (int rc = check_common(fn, p, nx, nz, ls)) return rc;
    if (int rc = check_members<T>(fn, ens, nx, nz, ls, m.nmem, m.ms)) return rc;
    if (shared)      // cloudsc2_nl_fused_enss_*
        if (int rc = check_shared<T>(fn, m, nx, nz, ls, in, eta, [&](auto&& hit) {
                for (int i = 0; out && i < NL_NUM_OUT; ++i) hit("out", i, out[i]);
                hit("qsat_out", 0, qsat_out);
            }))
            return rc;
    if (nx == 0) return CLOUDSC2_OK;   // empty call: nothing to check or launch (zero-size tensors carry NULL pointers)
    if (int rc = check_ptrs(fn, "out", const_cast<const T* const*>(out), NL_NUM_OUT)) return rc;
    if (!in) return fail(CLOUDSC2_E_ARG, "%s: in is NULL", fn);
    if (ens && (in_i || !qsat_out))
        return fail(CLOUDSC2_E_ARG, "%s: the ensemble entry is the saturation-fused form: qsat_out is required and in_i must "
                    "be NULL (the perturbed form has no ensemble kernel)", fn);
    if ((qsat_out != nullptr) == (in_i != nullptr))
        return fail(CLOUDSC2_E_ARG, "%s: exactly one of qsat_out (fused saturation) and in_i (fused perturbation) must be given", fn);
    for (int i = 0; i < NL_NUM_IN; ++i)
        if (!in[i] && !(qsat_out && i == NL_IN_QSAT)) return fail(CLOUDSC2_E_ARG, "%s: in[%d] is NULL", fn, i);
    if (in_i)
        if (int rc = check_ptrs(fn, "in_i", in_i, NL_NUM_IN)) return rc;
    if (!eta) return fail(CLOUDSC2_E_ARG, "%s: eta is NULL", fn);
    if (p->ICALL != 0) return fail(CLOUDSC2_E_UNSUPPORTED, "%s: ICALL=%d unsupported", fn, p->ICALL);
    if (qsat_out && !p->LPHYLIN)
        return fail(CLOUDSC2_E_UNSUPPORTED, "%s: only the LPHYLIN form of saturation is available fused", fn);
    if (!(dt > 0.0)) return fail(CLOUDSC2_E_ARG, "%s: dt=%g must be > 0", fn, dt);
    if (ens)
        return launched(fn, cs2::launch_nl_ens<T>(*p, nx, nz, ls, in, eta, out, dt, static_cast<hipStream_t>(stream), qsat_out,
                                                  m, shared));
    return launched(fn, cs2::launch_nl<T>(*p, nx, nz, ls, in, eta, out, dt, static_cast<hipStream_t>(stream), in_i, pf,
                                          qsat_out, nullptr));
}

// Perturbed NL run + Taylor-test reduction (build extension): see include/cloudsc2_hip.h.
template <typename T>
int nl_taylor_impl(const char* fn, const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const T* const* in,
                   const T* const* in_i, double pf, const T* eta, const T* const* ref_out, double* partials, double dt,
                   void* stream) {
    if (int rc = check_common(fn, p, nx, nz, ls)) return rc;
    if (nx == 0) return CLOUDSC2_OK;   // empty call: nothing to check or launch (zero-size tensors carry NULL pointers)
    if (int rc = check_ptrs(fn, "in", in, NL_NUM_IN)) return rc;
    if (int rc = check_ptrs(fn, "in_i", in_i, NL_NUM_IN)) return rc;
    if (int rc = check_ptrs(fn, "ref_out", ref_out, NL_NUM_OUT)) return rc;
    if (!eta) return fail(CLOUDSC2_E_ARG, "%s: eta is NULL", fn);
    if (!partials) return fail(CLOUDSC2_E_ARG, "%s: partials is NULL", fn);
    if (p->ICALL != 0) return fail(CLOUDSC2_E_UNSUPPORTED, "%s: ICALL=%d unsupported", fn, p->ICALL);
    if (!(dt > 0.0)) return fail(CLOUDSC2_E_ARG, "%s: dt=%g must be > 0", fn, dt);
    // the kernel only READS the reference outputs; the launcher's pointer pack is the mutable one
    T* refs[NL_NUM_OUT];
    for (int i = 0; i < NL_NUM_OUT; ++i) refs[i] = const_cast<T*>(ref_out[i]);
    return launched(fn, cs2::launch_nl<T>(*p, nx, nz, ls, in, eta, refs, dt, static_cast<hipStream_t>(stream), in_i, pf,
                                          nullptr, partials));
}

// The Taylor test's perturbed runs, several step sizes per launch (build extension): see include/cloudsc2_hip.h.
template <typename T>
int nl_taylor_multi_impl(const char* fn, const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const T* const* in,
                         const T* const* in_i, double inc_f, int32_t nf, const double* pf, const T* eta,
                         const T* const* ref_out, double* partials, double dt, void* stream) {
    if (int rc = check_common(fn, p, nx, nz, ls)) return rc;
    if (nf < 0 || nf > 64) return fail(CLOUDSC2_E_ARG, "%s: nf=%d outside [0, 64]", fn, nf);
    if (nx == 0 || nf == 0) return CLOUDSC2_OK;
    if (int rc = check_ptrs(fn, "in", in, NL_NUM_IN)) return rc;
    if (in_i)      // NULL: the increments are formed in the kernel as inc_f * in (state_increment fused in)
        if (int rc = check_ptrs(fn, "in_i", in_i, NL_NUM_IN)) return rc;
    if (int rc = check_ptrs(fn, "ref_out", ref_out, NL_NUM_OUT)) return rc;
    if (!eta) return fail(CLOUDSC2_E_ARG, "%s: eta is NULL", fn);
    if (!pf) return fail(CLOUDSC2_E_ARG, "%s: pf is NULL", fn);
    if (!partials) return fail(CLOUDSC2_E_ARG, "%s: partials is NULL", fn);
    if (p->ICALL != 0) return fail(CLOUDSC2_E_UNSUPPORTED, "%s: ICALL=%d unsupported", fn, p->ICALL);
    if (!(dt > 0.0)) return fail(CLOUDSC2_E_ARG, "%s: dt=%g must be > 0", fn, dt);
    if (nz > 2000) return fail(CLOUDSC2_E_UNSUPPORTED, "%s: nz=%d: the level table and the running sums must share the LDS", fn, nz);
    return launched(fn, cs2::launch_nl_taylor_multi<T>(*p, nx, nz, ls, in, in_i, nf, pf, eta, ref_out, partials, dt,
                                                       static_cast<hipStream_t>(stream), inc_f));
}

template <typename T>
int sums_impl(const char* fn, int32_t nx, int32_t nlev, int64_t ls, int32_t nf, const T* const* a, const T* const* b,
              double* partials, void* stream) {
    if (nx < 0 || nlev < 1 || ls < nx) return fail(CLOUDSC2_E_ARG, "%s: nx=%d nlev=%d lev_stride=%lld", fn, nx, nlev, (long long)ls);
    if (nf < 1 || nf > 16) return fail(CLOUDSC2_E_ARG, "%s: nfields=%d outside [1, 16]", fn, nf);
    if (nx == 0) return CLOUDSC2_OK;
    if (int rc = check_ptrs(fn, "a", a, nf)) return rc;
    if (b)
        if (int rc = check_ptrs(fn, "b", b, nf)) return rc;
    if (!partials) return fail(CLOUDSC2_E_ARG, "%s: partials is NULL", fn);
    return launched(fn, cs2::launch_field_sums<T>(nx, nlev, ls, nf, a, b, partials, static_cast<hipStream_t>(stream)));
}

template <typename T>
int dots_impl(const char* fn, int32_t nx, int32_t nlev, int64_t ls, int32_t np, const T* const* a, const T* const* b,
              double* out, int32_t accumulate, void* stream) {
    if (nx < 0 || nlev < 1 || ls < nx) return fail(CLOUDSC2_E_ARG, "%s: nx=%d nlev=%d lev_stride=%lld", fn, nx, nlev, (long long)ls);
    if (np < 1 || np > 16) return fail(CLOUDSC2_E_ARG, "%s: npairs=%d outside [1, 16]", fn, np);
    if (nx == 0) return CLOUDSC2_OK;
    if (int rc = check_ptrs(fn, "a", a, np)) return rc;
    if (int rc = check_ptrs(fn, "b", b, np)) return rc;
    if (!out) return fail(CLOUDSC2_E_ARG, "%s: out is NULL", fn);
    return launched(fn, cs2::launch_column_dots<T>(nx, nlev, ls, np, a, b, out, accumulate, static_cast<hipStream_t>(stream)));
}

// `fused_inc`: the state_increment-fused variant (cloudsc2_tl_incremented_*): in_i is absent, perturbations = inc_f * in
template <typename T>
int tl_impl(const char* fn, const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const T* const* in,
            const T* const* in_i, const T* eta, T* const* out, T* const* out_i, double dt, void* stream,
            bool fused_inc = false, double inc_f = 0.0) {
    if (int rc = check_common(fn, p, nx, nz, ls)) return rc;
    if (nx == 0) return CLOUDSC2_OK;   // empty call: nothing to check or launch (zero-size tensors carry NULL pointers)
    if (int rc = check_ptrs(fn, "in", in, NL_NUM_IN)) return rc;
    if (!fused_inc)
        if (int rc = check_ptrs(fn, "in_i", in_i, NL_NUM_IN)) return rc;
    if (int rc = check_ptrs(fn, "out", const_cast<const T* const*>(out), NL_NUM_OUT)) return rc;
    if (int rc = check_ptrs(fn, "out_i", const_cast<const T* const*>(out_i), NL_NUM_OUT)) return rc;
    if (!eta) return fail(CLOUDSC2_E_ARG, "%s: eta is NULL", fn);
    if (p->ICALL != 0) return fail(CLOUDSC2_E_UNSUPPORTED, "%s: ICALL=%d unsupported", fn, p->ICALL);
    if (!(dt > 0.0)) return fail(CLOUDSC2_E_ARG, "%s: dt=%g must be > 0", fn, dt);
    if (p->NLEV != nz) return fail(CLOUDSC2_E_ARG, "%s: NLEV=%d != nz=%d", fn, p->NLEV, nz);
    return launched(fn, cs2::launch_tl<T>(*p, nx, nz, ls, in, fused_inc ? nullptr : in_i, eta, out, out_i, dt,
                                          static_cast<hipStream_t>(stream), inc_f));
}

template <typename T>
int ad_impl(const char* fn, const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const T* const* in,
            const T* const* in_adj, const T* eta, T* const* out, T* const* out_adj, double dt, void* stream) {
    if (int rc = check_common(fn, p, nx, nz, ls)) return rc;
    if (nx == 0) return CLOUDSC2_OK;   // empty call: nothing to check or launch (zero-size tensors carry NULL pointers)
    if (int rc = check_ptrs(fn, "in", in, NL_NUM_IN)) return rc;
    if (int rc = check_ptrs(fn, "in_adj", in_adj, NL_NUM_OUT)) return rc;
    if (int rc = check_ptrs(fn, "out", const_cast<const T* const*>(out), NL_NUM_OUT)) return rc;
    if (int rc = check_ptrs(fn, "out_adj", const_cast<const T* const*>(out_adj), NL_NUM_IN)) return rc;
    if (!eta) return fail(CLOUDSC2_E_ARG, "%s: eta is NULL", fn);
    if (p->ICALL != 0) return fail(CLOUDSC2_E_UNSUPPORTED, "%s: ICALL=%d unsupported", fn, p->ICALL);
    if (!(dt > 0.0)) return fail(CLOUDSC2_E_ARG, "%s: dt=%g must be > 0", fn, dt);
    if (p->NLEV != nz) return fail(CLOUDSC2_E_ARG, "%s: NLEV=%d != nz=%d", fn, p->NLEV, nz);
    return launched(fn, cs2::launch_ad<T>(*p, nx, nz, ls, in, in_adj, eta, out, out_adj, dt, static_cast<hipStream_t>(stream),
                                          nullptr, nullptr));
}

template <typename T>
int ad_traj_impl(const char* fn, const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const T* const* in,
                 const T* const* in_adj, const T* eta, const T* traj_fplsl, const T* traj_fplsn, T* const* out_adj, double dt,
                 void* stream) {
    if (int rc = check_common(fn, p, nx, nz, ls)) return rc;
    if (nx == 0) return CLOUDSC2_OK;
    if (int rc = check_ptrs(fn, "in", in, NL_NUM_IN)) return rc;
    if (int rc = check_ptrs(fn, "in_adj", in_adj, NL_NUM_OUT)) return rc;
    if (int rc = check_ptrs(fn, "out_adj", const_cast<const T* const*>(out_adj), NL_NUM_IN)) return rc;
    if (!eta || !traj_fplsl || !traj_fplsn) return fail(CLOUDSC2_E_ARG, "%s: eta / traj_fplsl / traj_fplsn is NULL", fn);
    if (p->ICALL != 0) return fail(CLOUDSC2_E_UNSUPPORTED, "%s: ICALL=%d unsupported", fn, p->ICALL);
    if (p->LEVAPLS2 || p->LDRAIN1D)
        return fail(CLOUDSC2_E_UNSUPPORTED, "%s: the trajectory variant covers the driver switches only (no evaporation "
                    "block: its parked precipitation cover has no counterpart among the NL outputs) - use cloudsc2_ad", fn);
    if (!(dt > 0.0)) return fail(CLOUDSC2_E_ARG, "%s: dt=%g must be > 0", fn, dt);
    if (p->NLEV != nz) return fail(CLOUDSC2_E_ARG, "%s: NLEV=%d != nz=%d", fn, p->NLEV, nz);
    return launched(fn, cs2::launch_ad<T>(*p, nx, nz, ls, in, in_adj, eta, nullptr, out_adj, dt,
                                          static_cast<hipStream_t>(stream), traj_fplsl, traj_fplsn));
}

// ---- the masked TL / AD entries: NULL entries of in_i / in_adj are zero fields, NULL entries of out_i / out_adj are not
// written (include/cloudsc2_hip.h).  `what` names the array in messages.
template <typename T>
int check_masked_inputs(const char* fn, const char* what, const T* const* arr, int n, const T* zero_line) {
    if (!arr) return fail(CLOUDSC2_E_ARG, "%s: %s is NULL (the array itself; its entries may be)", fn, what);
    for (int i = 0; i < n; ++i)
        if (!arr[i] && !zero_line)
            return fail(CLOUDSC2_E_ARG, "%s: %s[%d] is NULL (a zero field) but zero_line is NULL too", fn, what, i);
    if (reinterpret_cast<uintptr_t>(zero_line) % 16)
        return fail(CLOUDSC2_E_ARG, "%s: zero_line is not 16-byte aligned", fn);
    return 0;
}

template <typename T>
int check_masked_outputs(const char* fn, const char* what, T* const* arr, int n) {
    if (!arr) return fail(CLOUDSC2_E_ARG, "%s: %s is NULL (the array itself; its entries may be)", fn, what);
    for (int i = 0; i < n; ++i)
        if (arr[i]) return 0;
    return fail(CLOUDSC2_E_ARG, "%s: every entry of %s is NULL: nothing would be written", fn, what);
}

template <typename T>
int check_masked_size(const char* fn, int32_t nz, int64_t ls) {
    if (cs2::fits_u32_offsets<T>(nz, ls)) return 0;
    return fail(CLOUDSC2_E_UNSUPPORTED,
                "%s: fields of 4 GiB or more ((nz+1) * lev_stride * sizeof(element) = %llu bytes >= 2^32): the masked "
                "kernels keep 32-bit byte offsets - use the dense stencil, or narrower allocations", fn,
                (unsigned long long)(nz + 1) * (unsigned long long)ls * sizeof(T));
}

// The step entries (cloudsc2_tl_step_* / cloudsc2_ad_step_*: `saturation` fused in): in[NL_IN_QSAT] is not read and may be
// NULL, every other trajectory field is required.
template <typename T>
int check_step_trajectory(const char* fn, const T* const* in) {
    if (!in) return fail(CLOUDSC2_E_ARG, "%s: in is NULL", fn);
    for (int i = 0; i < NL_NUM_IN; ++i)
        if (!in[i] && i != NL_IN_QSAT) return fail(CLOUDSC2_E_ARG, "%s: in[%d] is NULL", fn, i);
    return 0;
}

int check_step_saturation(const char* fn, const Cloudsc2Params* p) {
    if (p->LPHYLIN) return 0;
    return fail(CLOUDSC2_E_UNSUPPORTED, "%s: only the LPHYLIN form of saturation is available fused (use "
                "cloudsc2_saturation_tl / _ad with the masked entries for the other forms)", fn);
}

// the direction arguments of the cloudsc2_tl_multi_* / cloudsc2_ad_multi_* entries
int check_dirs(const char* fn, int32_t nz, int64_t ls, const cs2::CallDirs& d, int max_dirs, const char* max_name) {
    if (d.ndir < 1 || d.ndir > max_dirs)
        return fail(CLOUDSC2_E_ARG, "%s: ndir=%d outside [1, %d] (%s)", fn, d.ndir, max_dirs, max_name);
    const int64_t field = int64_t(nz + 1) * ls;
    if (d.in_ds < field || d.out_ds < field)
        return fail(CLOUDSC2_E_ARG, "%s: in_dir_stride=%lld / out_dir_stride=%lld < (nz+1) * lev_stride = %lld: the "
                    "directions of a field would overlap", fn, (long long)d.in_ds, (long long)d.out_ds, (long long)field);
    return 0;
}

// The two further member strides of the cloudsc2_ad_multi_ens_* / cloudsc2_ad_multi_step_ens_* entries (check_dirs and
// check_members have passed): member-major batches only - the directions of one member lie inside its member stride
int check_member_batches(const char* fn, int32_t nz, int64_t ls, const cs2::CallDirs& d, const cs2::CallMembers& m) {
    const int64_t field = int64_t(nz + 1) * ls;
    // (ndir-1) * dir_stride + field <= member_stride, by division: the strides are the caller's and their product may overflow
    const auto fits = [&](int64_t ms, int64_t ds) {
        return ms >= field && (d.ndir == 1 || ds <= (ms - field) / (d.ndir - 1));
    };
    if (!fits(m.in_ms, d.in_ds))
        return fail(CLOUDSC2_E_ARG, "%s: in_member_stride=%lld < (ndir-1) * in_dir_stride + (nz+1) * lev_stride (ndir=%d, "
                    "in_dir_stride=%lld, (nz+1) * lev_stride=%lld): the batches are member-major, a member's directions must "
                    "not reach into the next member", fn, (long long)m.in_ms, d.ndir, (long long)d.in_ds, (long long)field);
    if (!fits(m.out_ms, d.out_ds))
        return fail(CLOUDSC2_E_ARG, "%s: out_member_stride=%lld < (ndir-1) * out_dir_stride + (nz+1) * lev_stride (ndir=%d, "
                    "out_dir_stride=%lld, (nz+1) * lev_stride=%lld): the batches are member-major, a member's directions must "
                    "not reach into the next member", fn, (long long)m.out_ms, d.ndir, (long long)d.out_ds, (long long)field);
    return 0;
}

// The form of the entry (cs2::CallForm) - kStep: the cloudsc2_tl_step_* entry (tl_step_kernel); kMulti: the
// cloudsc2_tl_multi_* entries (tl_dirs_kernel); kEns: the cloudsc2_tl_ens_* / cloudsc2_tl_step_ens_* entries (tl_ens_kernel /
// tl_ens_step_kernel)
template <typename T>
int tl_masked_impl(const char* fn, const cs2::TLCall<T>& c) {
    const bool step = c.is(cs2::kStep), multi = c.is(cs2::kMulti);
    const Cloudsc2Params* const p = c.p;
    if (int rc = check_common(fn, p, c.nx, c.nz, c.ls)) return rc;
    if (multi)
        if (int rc = check_dirs(fn, c.nz, c.ls, c.dirs, CLOUDSC2_TL_MAX_DIRS, "CLOUDSC2_TL_MAX_DIRS")) return rc;
    if (int rc = check_members<T>(fn, c.is(cs2::kEns), c.nx, c.nz, c.ls, c.members.nmem, c.members.ms)) return rc;
    if (c.is(cs2::kShared))   // cloudsc2_tl_enss_* / cloudsc2_tl_step_enss_* (tl_enss_kernel / tl_enss_step_kernel)
        if (int rc = check_shared<T>(fn, c.members, c.nx, c.nz, c.ls, c.in, c.eta, [&](auto&& hit) {
                for (int i = 0; c.out && i < NL_NUM_OUT; ++i) hit("out", i, c.out[i]);
                for (int i = 0; c.out_i && i < NL_NUM_OUT; ++i) hit("out_i", i, c.out_i[i]);
            }))
            return rc;
    if (c.nx == 0) return CLOUDSC2_OK;
    if (int rc = step ? check_step_trajectory(fn, c.in) : check_ptrs(fn, "in", c.in, NL_NUM_IN)) return rc;
    if (step && c.in_i && c.in_i[NL_IN_QSAT])
        return fail(CLOUDSC2_E_ARG, "%s: in_i[NL_IN_QSAT] (in_i[%d]) must be NULL: the qsat perturbation is formed in the "
                    "kernel from in_i[NL_IN_T] and in_i[NL_IN_AP] (use cloudsc2_tl_masked for an independent one)", fn,
                    NL_IN_QSAT);
    if (step && c.in_i && !c.zero) {       // the one NULL entry that needs no zero line: it is not read at all
        for (int i = 0; i < NL_NUM_IN; ++i)
            if (!c.in_i[i] && i != NL_IN_QSAT)
                return fail(CLOUDSC2_E_ARG, "%s: in_i[%d] is NULL (a zero field) but zero_line is NULL too", fn, i);
    } else if (int rc = check_masked_inputs(fn, "in_i", c.in_i, NL_NUM_IN, c.zero)) {
        return rc;
    }
    if (c.out)
        if (int rc = check_ptrs(fn, "out (all ten entries, or the array itself NULL)", const_cast<const T* const*>(c.out), NL_NUM_OUT))
            return rc;
    if (int rc = check_masked_outputs(fn, "out_i", c.out_i, NL_NUM_OUT)) return rc;
    if (!c.eta) return fail(CLOUDSC2_E_ARG, "%s: eta is NULL", fn);
    if (p->ICALL != 0) return fail(CLOUDSC2_E_UNSUPPORTED, "%s: ICALL=%d unsupported", fn, p->ICALL);
    if (!(c.dt > 0.0)) return fail(CLOUDSC2_E_ARG, "%s: dt=%g must be > 0", fn, c.dt);
    if (p->NLEV != c.nz) return fail(CLOUDSC2_E_ARG, "%s: NLEV=%d != nz=%d", fn, p->NLEV, c.nz);
    if (step)
        if (int rc = check_step_saturation(fn, p)) return rc;
    if (int rc = check_masked_size<T>(fn, c.nz, c.ls)) return rc;
    return launched(fn, multi ? cs2::launch_tl_dirs<T>(c) : cs2::launch_tl_masked<T>(c));
}

// The evaporation ensemble entries: sweep 1 WRITES `cover` while every other field of the call is read (or written by sweep
// 2), so a `cover` that shares storage with one of them is refused (member_ranges_overlap, above).
template <typename T>
int check_cover_disjoint(const char* fn, const cs2::ADCall<T>& c) {
    const int64_t nmem = c.members.nmem;
    const int64_t ext = (int64_t(c.nz) * c.ls + c.nx) * int64_t(sizeof(T)), sb = c.members.ms * int64_t(sizeof(T));
    const auto hits = [&](const T* f, int64_t ef, int64_t nf) {
        return f && member_ranges_overlap(c.cover.cover, ext, nmem, f, ef, nf, sb);
    };
    const auto refuse = [&](const char* what, int i) {
        return fail(CLOUDSC2_E_ARG, "%s: cover overlaps %s[%d] in some member: cover must not share storage with any other "
                    "field of the call", fn, what, i);
    };
    for (int i = 0; i < NL_NUM_IN; ++i) {
        if (hits(c.in[i], ext, nmem)) return refuse("in", i);
        if (hits(c.out_adj[i], ext, nmem)) return refuse("out_adj", i);
    }
    for (int i = 0; i < NL_NUM_OUT; ++i)
        if (hits(c.in_adj[i], ext, nmem)) return refuse("in_adj", i);
    if (hits(c.traj_l, ext, nmem) || hits(c.traj_n, ext, nmem)) return refuse("traj_fplsl / traj_fplsn", 0);
    if (hits(c.zero, 512, 1)) return refuse("zero_line", 0);
    if (hits(c.eta, int64_t(c.nz + 1) * int64_t(sizeof(T)), 1)) return refuse("eta", 0);
    return 0;
}

// The form of the entry (cs2::CallForm) - kStep: the cloudsc2_ad_step_* entry (ad_step_kernel); kMulti: the
// cloudsc2_ad_multi_* entries (ad_dirs_kernel); kEns: the cloudsc2_ad_ens_* / cloudsc2_ad_step_ens_* entries (ad_ens_kernel /
// ad_ens_step_kernel); kMulti and kEns: cloudsc2_ad_multi_ens_* / _multi_step_ens_* (ad_mdirs_kernel / ad_mdirs_step_kernel),
// members times directions; kEvap: the trajectory adjoints WITH the evaporation block (cloudsc2_ad_evap_* / _step_* / _multi_* /
// _multi_step_*: ad_cover_kernel and its siblings) - the same checks, the switches required instead of refused, and the
// caller's cover field; kEvap and kEns: cloudsc2_ad_evap_ens_* / _step_ens_* (ad_cover_ens_kernel / ad_cover_ens_step_kernel),
// `cover` batched too.
template <typename T>
int ad_masked_impl(const char* fn, const cs2::ADCall<T>& c) {
    const bool step = c.is(cs2::kStep), multi = c.is(cs2::kMulti), ens = c.is(cs2::kEns), evap = c.is(cs2::kEvap);
    const Cloudsc2Params* const p = c.p;
    if (int rc = check_common(fn, p, c.nx, c.nz, c.ls)) return rc;
    if (multi)
        if (int rc = check_dirs(fn, c.nz, c.ls, c.dirs, CLOUDSC2_AD_MAX_DIRS, "CLOUDSC2_AD_MAX_DIRS")) return rc;
    if (int rc = check_members<T>(fn, ens, c.nx, c.nz, c.ls, c.members.nmem, c.members.ms)) return rc;
    if (multi && ens)
        if (int rc = check_member_batches(fn, c.nz, c.ls, c.dirs, c.members)) return rc;
    if (c.is(cs2::kShared))   // cloudsc2_ad_enss_* / cloudsc2_ad_step_enss_* (ad_enss_kernel / ad_enss_step_kernel)
        if (int rc = check_shared<T>(fn, c.members, c.nx, c.nz, c.ls, c.in, c.eta, [&](auto&& hit) {
                for (int i = 0; c.out_adj && i < NL_NUM_IN; ++i) hit("out_adj", i, c.out_adj[i]);
            }))
            return rc;
    if (c.nx == 0) return CLOUDSC2_OK;
    if (int rc = step ? check_step_trajectory(fn, c.in) : check_ptrs(fn, "in", c.in, NL_NUM_IN)) return rc;
    if (int rc = check_masked_inputs(fn, "in_adj", c.in_adj, NL_NUM_OUT, c.zero)) return rc;
    if (step && c.out_adj && c.out_adj[NL_IN_QSAT])
        return fail(CLOUDSC2_E_ARG, "%s: out_adj[NL_IN_QSAT] (out_adj[%d]) must be NULL: the qsat adjoint is folded into "
                    "out_adj[NL_IN_T] and out_adj[NL_IN_AP] (use cloudsc2_ad_%s to have it stored)", fn, NL_IN_QSAT,
                    evap ? "evap" : "masked");
    if (int rc = check_masked_outputs(fn, "out_adj", c.out_adj, NL_NUM_IN)) return rc;
    if (!c.eta || !c.traj_l || !c.traj_n) return fail(CLOUDSC2_E_ARG, "%s: eta / traj_fplsl / traj_fplsn is NULL", fn);
    if (evap && !c.cover.cover)
        return fail(CLOUDSC2_E_ARG, "%s: cover is NULL (a caller-owned field of nz+1 levels at lev_stride)", fn);
    if (p->ICALL != 0) return fail(CLOUDSC2_E_UNSUPPORTED, "%s: ICALL=%d unsupported", fn, p->ICALL);
    if (!evap && (p->LEVAPLS2 || p->LDRAIN1D))
        return fail(CLOUDSC2_E_UNSUPPORTED, "%s: LEVAPLS2 / LDRAIN1D: the masked adjoint reads its trajectory like "
                    "cloudsc2_ad_from_trajectory and covers the driver switches only (the evaporation block's parked "
                    "precipitation cover has no counterpart among the NL outputs) - use cloudsc2_ad", fn);
    if (evap && !(p->LEVAPLS2 || p->LDRAIN1D))
        return fail(CLOUDSC2_E_UNSUPPORTED, "%s: neither LEVAPLS2 nor LDRAIN1D is set: without the evaporation block there is "
                    "no precipitation cover to carry - use cloudsc2_ad_%s", fn,
                    ens ? (step ? "step_ens" : "ens") : multi ? (step ? "multi_step" : "multi") : (step ? "step" : "masked"));
    if (!(c.dt > 0.0)) return fail(CLOUDSC2_E_ARG, "%s: dt=%g must be > 0", fn, c.dt);
    if (p->NLEV != c.nz) return fail(CLOUDSC2_E_ARG, "%s: NLEV=%d != nz=%d", fn, p->NLEV, c.nz);
    if (step)
        if (int rc = check_step_saturation(fn, p)) return rc;
    if (int rc = check_masked_size<T>(fn, c.nz, c.ls)) return rc;
    if (evap && ens)
        if (int rc = check_cover_disjoint<T>(fn, c)) return rc;
    return launched(fn, evap ? cs2::launch_ad_cover<T>(c) : multi ? cs2::launch_ad_dirs<T>(c) : cs2::launch_ad_masked<T>(c));
}

template <typename T>
int sat_impl(const char* fn, const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const T* ap, const T* t,
             T* qsat, void* stream) {
    if (int rc = check_common(fn, p, nx, nz, ls)) return rc;
    if (nx == 0) return CLOUDSC2_OK;   // empty call: nothing to check or launch (zero-size tensors carry NULL pointers)
    if (!ap || !t || !qsat) return fail(CLOUDSC2_E_ARG, "%s: NULL field pointer", fn);
    return launched(fn, cs2::launch_saturation<T>(*p, nx, nz, ls, ap, t, qsat, static_cast<hipStream_t>(stream)));
}

// tangent-linear / adjoint of `saturation` (build extensions): see include/cloudsc2_hip.h
template <typename T>
int sat_tl_impl(const char* fn, const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const T* ap, const T* t,
                const T* ap_i, const T* t_i, T* qsat, T* qsat_i, void* stream) {
    if (int rc = check_common(fn, p, nx, nz, ls)) return rc;
    if (nx == 0) return CLOUDSC2_OK;
    if (!ap) return fail(CLOUDSC2_E_ARG, "%s: ap is NULL", fn);
    if (!t) return fail(CLOUDSC2_E_ARG, "%s: t is NULL", fn);
    if (!ap_i && !t_i) return fail(CLOUDSC2_E_ARG, "%s: ap_i and t_i are both NULL: there is nothing to propagate", fn);
    if (!qsat_i) return fail(CLOUDSC2_E_ARG, "%s: qsat_i is NULL", fn);
    return launched(fn, cs2::launch_saturation_tl<T>(*p, nx, nz, ls, ap, t, ap_i, t_i, qsat, qsat_i,
                                                     static_cast<hipStream_t>(stream)));
}

template <typename T>
int sat_ad_impl(const char* fn, const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const T* ap, const T* t,
                const T* qsat_adj, T* ap_adj, T* t_adj, int32_t accumulate, void* stream) {
    if (int rc = check_common(fn, p, nx, nz, ls)) return rc;
    if (nx == 0) return CLOUDSC2_OK;
    if (!ap) return fail(CLOUDSC2_E_ARG, "%s: ap is NULL", fn);
    if (!t) return fail(CLOUDSC2_E_ARG, "%s: t is NULL", fn);
    if (!qsat_adj) return fail(CLOUDSC2_E_ARG, "%s: qsat_adj is NULL", fn);
    if (!ap_adj && !t_adj) return fail(CLOUDSC2_E_ARG, "%s: ap_adj and t_adj are both NULL: nothing would be written", fn);
    return launched(fn, cs2::launch_saturation_ad<T>(*p, nx, nz, ls, ap, t, qsat_adj, ap_adj, t_adj, accumulate,
                                                     static_cast<hipStream_t>(stream)));
}

template <typename T>
int inc_impl(const char* fn, const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const T* const* in,
             T* const* out, double f, void* stream) {
    if (int rc = check_common(fn, p, nx, nz, ls)) return rc;
    if (nx == 0) return CLOUDSC2_OK;   // empty call: nothing to check or launch (zero-size tensors carry NULL pointers)
    if (int rc = check_ptrs(fn, "in", in, INC_NUM)) return rc;
    if (int rc = check_ptrs(fn, "out_i", const_cast<const T* const*>(out), INC_NUM)) return rc;
    return launched(fn, cs2::launch_increment<T>(*p, nx, nz, ls, in, out, f, static_cast<hipStream_t>(stream)));
}

template <typename T>
int per_impl(const char* fn, const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const T* const* in,
             const T* const* in_i, T* const* out, double f, void* stream) {
    if (int rc = check_common(fn, p, nx, nz, ls)) return rc;
    if (nx == 0) return CLOUDSC2_OK;   // empty call: nothing to check or launch (zero-size tensors carry NULL pointers)
    if (int rc = check_ptrs(fn, "in", in, INC_NUM)) return rc;
    if (int rc = check_ptrs(fn, "in_i", in_i, INC_NUM)) return rc;
    if (int rc = check_ptrs(fn, "out", const_cast<const T* const*>(out), INC_NUM)) return rc;
    return launched(fn, cs2::launch_perturb<T>(nx, nz, ls, in, in_i, out, f, static_cast<hipStream_t>(stream)));
}

}  // namespace

namespace cs2 {
void note_kernel(const char* name) { g_kernel.store(name, std::memory_order_relaxed); }
}  // namespace cs2

extern "C" {

int32_t cloudsc2_abi_version(void) { return CLOUDSC2_ABI_VERSION; }
int32_t cloudsc2_params_sizeof(void) { return (int32_t)sizeof(Cloudsc2Params); }
const char* cloudsc2_last_error(void) { return g_err; }
const char* cloudsc2_last_kernel(void) { return g_kernel.load(std::memory_order_relaxed); }
int32_t cloudsc2_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int32_t cloudsc2_nl_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const double* const* in,
                        const double* eta, double* const* out, double dt, void* stream) {
    return nl_impl<double>("cloudsc2_nl_f64", p, nx, nz, ls, in, eta, out, dt, stream);
}
int32_t cloudsc2_nl_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const float* const* in,
                        const float* eta, float* const* out, double dt, void* stream) {
    return nl_impl<float>("cloudsc2_nl_f32", p, nx, nz, ls, in, eta, out, dt, stream);
}
int32_t cloudsc2_nl_fused_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const double* const* in,
                              const double* const* in_i, double pf, double* qsat_out, const double* eta,
                              double* const* out, double dt, void* stream) {
    return nl_fused_impl<double>("cloudsc2_nl_fused_f64", p, nx, nz, ls, in, in_i, pf, qsat_out, eta, out, dt, stream);
}
int32_t cloudsc2_nl_fused_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const float* const* in,
                              const float* const* in_i, double pf, float* qsat_out, const float* eta,
                              float* const* out, double dt, void* stream) {
    return nl_fused_impl<float>("cloudsc2_nl_fused_f32", p, nx, nz, ls, in, in_i, pf, qsat_out, eta, out, dt, stream);
}
int32_t cloudsc2_nl_taylor_blocks(int32_t nx) { return nx <= 0 ? 0 : (nx + cs2::kColBlock - 1) / cs2::kColBlock; }
int32_t cloudsc2_nl_taylor_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const double* const* in,
                               const double* const* in_i, double pf, const double* eta, const double* const* ref_out,
                               double* partials, double dt, void* stream) {
    return nl_taylor_impl<double>("cloudsc2_nl_taylor_f64", p, nx, nz, ls, in, in_i, pf, eta, ref_out, partials, dt, stream);
}
int32_t cloudsc2_nl_taylor_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const float* const* in,
                               const float* const* in_i, double pf, const float* eta, const float* const* ref_out,
                               double* partials, double dt, void* stream) {
    return nl_taylor_impl<float>("cloudsc2_nl_taylor_f32", p, nx, nz, ls, in, in_i, pf, eta, ref_out, partials, dt, stream);
}
int32_t cloudsc2_nl_taylor_multi_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const double* const* in,
                                     const double* const* in_i, double inc_f, int32_t nf, const double* pf, const double* eta,
                                     const double* const* ref_out, double* partials, double dt, void* stream) {
    return nl_taylor_multi_impl<double>("cloudsc2_nl_taylor_multi_f64", p, nx, nz, ls, in, in_i, inc_f, nf, pf, eta, ref_out,
                                        partials, dt, stream);
}
int32_t cloudsc2_nl_taylor_multi_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const float* const* in,
                                     const float* const* in_i, double inc_f, int32_t nf, const double* pf, const float* eta,
                                     const float* const* ref_out, double* partials, double dt, void* stream) {
    return nl_taylor_multi_impl<float>("cloudsc2_nl_taylor_multi_f32", p, nx, nz, ls, in, in_i, inc_f, nf, pf, eta, ref_out,
                                       partials, dt, stream);
}
int32_t cloudsc2_field_sums_blocks(int32_t nx, int32_t nlev) { return cs2::field_sums_blocks(nx, nlev); }
int32_t cloudsc2_column_dots_chunks(int32_t nlev) { return cs2::column_dots_chunks(nlev); }
int32_t cloudsc2_field_sums_f64(int32_t nx, int32_t nlev, int64_t ls, int32_t nf, const double* const* a,
                                const double* const* b, double* partials, void* stream) {
    return sums_impl<double>("cloudsc2_field_sums_f64", nx, nlev, ls, nf, a, b, partials, stream);
}
int32_t cloudsc2_field_sums_f32(int32_t nx, int32_t nlev, int64_t ls, int32_t nf, const float* const* a,
                                const float* const* b, double* partials, void* stream) {
    return sums_impl<float>("cloudsc2_field_sums_f32", nx, nlev, ls, nf, a, b, partials, stream);
}
int32_t cloudsc2_column_dots_f64(int32_t nx, int32_t nlev, int64_t ls, int32_t np, const double* const* a,
                                 const double* const* b, double* out, int32_t accumulate, void* stream) {
    return dots_impl<double>("cloudsc2_column_dots_f64", nx, nlev, ls, np, a, b, out, accumulate, stream);
}
int32_t cloudsc2_column_dots_f32(int32_t nx, int32_t nlev, int64_t ls, int32_t np, const float* const* a,
                                 const float* const* b, double* out, int32_t accumulate, void* stream) {
    return dots_impl<float>("cloudsc2_column_dots_f32", nx, nlev, ls, np, a, b, out, accumulate, stream);
}
int32_t cloudsc2_tl_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const double* const* in,
                        const double* const* in_i, const double* eta, double* const* out, double* const* out_i,
                        double dt, void* stream) {
    return tl_impl<double>("cloudsc2_tl_f64", p, nx, nz, ls, in, in_i, eta, out, out_i, dt, stream);
}
int32_t cloudsc2_tl_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const float* const* in,
                        const float* const* in_i, const float* eta, float* const* out, float* const* out_i,
                        double dt, void* stream) {
    return tl_impl<float>("cloudsc2_tl_f32", p, nx, nz, ls, in, in_i, eta, out, out_i, dt, stream);
}
int32_t cloudsc2_tl_incremented_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const double* const* in,
                                    double f, const double* eta, double* const* out, double* const* out_i, double dt,
                                    void* stream) {
    return tl_impl<double>("cloudsc2_tl_incremented_f64", p, nx, nz, ls, in, nullptr, eta, out, out_i, dt, stream, true, f);
}
int32_t cloudsc2_tl_incremented_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const float* const* in,
                                    double f, const float* eta, float* const* out, float* const* out_i, double dt,
                                    void* stream) {
    return tl_impl<float>("cloudsc2_tl_incremented_f32", p, nx, nz, ls, in, nullptr, eta, out, out_i, dt, stream, true, f);
}
int32_t cloudsc2_ad_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const double* const* in,
                        const double* const* in_adj, const double* eta, double* const* out,
                        double* const* out_adj, double dt, void* stream) {
    return ad_impl<double>("cloudsc2_ad_f64", p, nx, nz, ls, in, in_adj, eta, out, out_adj, dt, stream);
}
int32_t cloudsc2_ad_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const float* const* in,
                        const float* const* in_adj, const float* eta, float* const* out, float* const* out_adj,
                        double dt, void* stream) {
    return ad_impl<float>("cloudsc2_ad_f32", p, nx, nz, ls, in, in_adj, eta, out, out_adj, dt, stream);
}
int32_t cloudsc2_ad_from_trajectory_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const double* const* in,
                                        const double* const* in_adj, const double* eta, const double* traj_fplsl,
                                        const double* traj_fplsn, double* const* out_adj, double dt, void* stream) {
    return ad_traj_impl<double>("cloudsc2_ad_from_trajectory_f64", p, nx, nz, ls, in, in_adj, eta, traj_fplsl, traj_fplsn,
                                out_adj, dt, stream);
}
int32_t cloudsc2_ad_from_trajectory_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const float* const* in,
                                        const float* const* in_adj, const float* eta, const float* traj_fplsl,
                                        const float* traj_fplsn, float* const* out_adj, double dt, void* stream) {
    return ad_traj_impl<float>("cloudsc2_ad_from_trajectory_f32", p, nx, nz, ls, in, in_adj, eta, traj_fplsl, traj_fplsn,
                               out_adj, dt, stream);
}
int32_t cloudsc2_saturation_tl_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const double* ap,
                                   const double* t, const double* ap_i, const double* t_i, double* qsat, double* qsat_i, void* stream) {
    return sat_tl_impl<double>("cloudsc2_saturation_tl_f64", p, nx, nz, ls, ap, t, ap_i, t_i, qsat, qsat_i, stream);
}
int32_t cloudsc2_saturation_ad_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const double* ap,
                                   const double* t, const double* qsat_adj, double* ap_adj, double* t_adj, int32_t accumulate,
                                   void* stream) {
    return sat_ad_impl<double>("cloudsc2_saturation_ad_f64", p, nx, nz, ls, ap, t, qsat_adj, ap_adj, t_adj, accumulate, stream);
}
int32_t cloudsc2_saturation_tl_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const float* ap,
                                   const float* t, const float* ap_i, const float* t_i, float* qsat, float* qsat_i, void* stream) {
    return sat_tl_impl<float>("cloudsc2_saturation_tl_f32", p, nx, nz, ls, ap, t, ap_i, t_i, qsat, qsat_i, stream);
}
int32_t cloudsc2_saturation_ad_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const float* ap,
                                   const float* t, const float* qsat_adj, float* ap_adj, float* t_adj, int32_t accumulate,
                                   void* stream) {
    return sat_ad_impl<float>("cloudsc2_saturation_ad_f32", p, nx, nz, ls, ap, t, qsat_adj, ap_adj, t_adj, accumulate, stream);
}
int32_t cloudsc2_saturation_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const double* ap,
                                const double* t, double* qsat, void* stream) {
    return sat_impl<double>("cloudsc2_saturation_f64", p, nx, nz, ls, ap, t, qsat, stream);
}
int32_t cloudsc2_saturation_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const float* ap,
                                const float* t, float* qsat, void* stream) {
    return sat_impl<float>("cloudsc2_saturation_f32", p, nx, nz, ls, ap, t, qsat, stream);
}
int32_t cloudsc2_state_increment_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls,
                                     const double* const* in, double* const* out_i, double f, void* stream) {
    return inc_impl<double>("cloudsc2_state_increment_f64", p, nx, nz, ls, in, out_i, f, stream);
}
int32_t cloudsc2_state_increment_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls,
                                     const float* const* in, float* const* out_i, double f, void* stream) {
    return inc_impl<float>("cloudsc2_state_increment_f32", p, nx, nz, ls, in, out_i, f, stream);
}
int32_t cloudsc2_perturbed_state_f64(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls,
                                     const double* const* in, const double* const* in_i, double* const* out,
                                     double f, void* stream) {
    return per_impl<double>("cloudsc2_perturbed_state_f64", p, nx, nz, ls, in, in_i, out, f, stream);
}
int32_t cloudsc2_perturbed_state_f32(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls,
                                     const float* const* in, const float* const* in_i, float* const* out,
                                     double f, void* stream) {
    return per_impl<float>("cloudsc2_perturbed_state_f32", p, nx, nz, ls, in, in_i, out, f, stream);
}
// ---- the masked TL / AD family, all twenty-eight entries once per precision.  Every wrapper builds the call descriptor from its own
// arguments: the head and the arrays by CS2_TL_CALL / CS2_AD_CALL under the entry's form, then the groups the entry has.
#define CS2_TL_ARGS(T)                                                                                                         \
    const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const T* const* in, const T* const* in_i, const T* zero_line, \
        const T* eta, T* const* out, T* const* out_i, double dt
#define CS2_AD_ARGS(T)                                                                                                         \
    const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const T* const* in, const T* const* in_adj,                   \
        const T* zero_line, const T* eta, const T* traj_fplsl, const T* traj_fplsn, T* const* out_adj, double dt
#define CS2_DIRS_ARGS int32_t ndir, int64_t in_ds, int64_t out_ds
#define CS2_ENS_ARGS int32_t nmem, int64_t ms
#define CS2_ENSS_ARGS int32_t nmem, int64_t ms, int64_t shared_mask, int64_t eta_ms
#define CS2_MENS_ARGS int32_t nmem, int64_t ms, int64_t in_ms, int64_t out_ms
#define CS2_COVER_ARGS(T) T* cover, int32_t cover_ready
#define CS2_TL_CALL(T, FORM)                                                                                                   \
    cs2::TLCall<T> c{{p, nx, nz, ls, in, zero_line, eta, dt, static_cast<hipStream_t>(stream), FORM}, in_i, out, out_i}
#define CS2_AD_CALL(T, FORM)                                                                                                   \
    cs2::ADCall<T> c{{p, nx, nz, ls, in, zero_line, eta, dt, static_cast<hipStream_t>(stream), FORM},                          \
                     in_adj, traj_fplsl, traj_fplsn, out_adj}
#define CS2_DIRS c.dirs = {ndir, in_ds, out_ds}
#define CS2_ENS c.members = {nmem, ms}
#define CS2_ENSS_MEMBERS {nmem, ms, 0, 0, shared_mask, eta_ms}
#define CS2_ENSS c.members = CS2_ENSS_MEMBERS
#define CS2_MENS c.members = {nmem, ms, in_ms, out_ms}
#define CS2_COVER c.cover = {cover, cover_ready}
#define CS2_MASKED_ENTRIES(SFX, T)                                                                                             \
    int32_t cloudsc2_tl_masked_##SFX(CS2_TL_ARGS(T), void* stream) {                                                           \
        CS2_TL_CALL(T, cs2::kMasked);                                                                                          \
        return tl_masked_impl<T>("cloudsc2_tl_masked_" #SFX, c);                                                               \
    }                                                                                                                          \
    int32_t cloudsc2_tl_step_##SFX(CS2_TL_ARGS(T), void* stream) {                                                             \
        CS2_TL_CALL(T, cs2::kStep);                                                                                            \
        return tl_masked_impl<T>("cloudsc2_tl_step_" #SFX, c);                                                                 \
    }                                                                                                                          \
    int32_t cloudsc2_tl_multi_##SFX(CS2_TL_ARGS(T), void* stream, CS2_DIRS_ARGS) {                                             \
        CS2_TL_CALL(T, cs2::kMulti);                                                                                           \
        CS2_DIRS;                                                                                                              \
        return tl_masked_impl<T>("cloudsc2_tl_multi_" #SFX, c);                                                                \
    }                                                                                                                          \
    int32_t cloudsc2_tl_multi_step_##SFX(CS2_TL_ARGS(T), void* stream, CS2_DIRS_ARGS) {                                        \
        CS2_TL_CALL(T, cs2::kStep | cs2::kMulti);                                                                              \
        CS2_DIRS;                                                                                                              \
        return tl_masked_impl<T>("cloudsc2_tl_multi_step_" #SFX, c);                                                           \
    }                                                                                                                          \
    int32_t cloudsc2_tl_ens_##SFX(CS2_TL_ARGS(T), void* stream, CS2_ENS_ARGS) {                                                \
        CS2_TL_CALL(T, cs2::kEns);                                                                                             \
        CS2_ENS;                                                                                                               \
        return tl_masked_impl<T>("cloudsc2_tl_ens_" #SFX, c);                                                                  \
    }                                                                                                                          \
    int32_t cloudsc2_tl_step_ens_##SFX(CS2_TL_ARGS(T), void* stream, CS2_ENS_ARGS) {                                           \
        CS2_TL_CALL(T, cs2::kStep | cs2::kEns);                                                                                \
        CS2_ENS;                                                                                                               \
        return tl_masked_impl<T>("cloudsc2_tl_step_ens_" #SFX, c);                                                             \
    }                                                                                                                          \
    int32_t cloudsc2_ad_masked_##SFX(CS2_AD_ARGS(T), void* stream) {                                                           \
        CS2_AD_CALL(T, cs2::kMasked);                                                                                          \
        return ad_masked_impl<T>("cloudsc2_ad_masked_" #SFX, c);                                                               \
    }                                                                                                                          \
    int32_t cloudsc2_ad_step_##SFX(CS2_AD_ARGS(T), void* stream) {                                                             \
        CS2_AD_CALL(T, cs2::kStep);                                                                                            \
        return ad_masked_impl<T>("cloudsc2_ad_step_" #SFX, c);                                                                 \
    }                                                                                                                          \
    int32_t cloudsc2_ad_multi_##SFX(CS2_AD_ARGS(T), void* stream, CS2_DIRS_ARGS) {                                             \
        CS2_AD_CALL(T, cs2::kMulti);                                                                                           \
        CS2_DIRS;                                                                                                              \
        return ad_masked_impl<T>("cloudsc2_ad_multi_" #SFX, c);                                                                \
    }                                                                                                                          \
    int32_t cloudsc2_ad_multi_step_##SFX(CS2_AD_ARGS(T), void* stream, CS2_DIRS_ARGS) {                                        \
        CS2_AD_CALL(T, cs2::kStep | cs2::kMulti);                                                                              \
        CS2_DIRS;                                                                                                              \
        return ad_masked_impl<T>("cloudsc2_ad_multi_step_" #SFX, c);                                                           \
    }                                                                                                                          \
    int32_t cloudsc2_ad_ens_##SFX(CS2_AD_ARGS(T), void* stream, CS2_ENS_ARGS) {                                                \
        CS2_AD_CALL(T, cs2::kEns);                                                                                             \
        CS2_ENS;                                                                                                               \
        return ad_masked_impl<T>("cloudsc2_ad_ens_" #SFX, c);                                                                  \
    }                                                                                                                          \
    int32_t cloudsc2_ad_step_ens_##SFX(CS2_AD_ARGS(T), void* stream, CS2_ENS_ARGS) {                                           \
        CS2_AD_CALL(T, cs2::kStep | cs2::kEns);                                                                                \
        CS2_ENS;                                                                                                               \
        return ad_masked_impl<T>("cloudsc2_ad_step_ens_" #SFX, c);                                                             \
    }                                                                                                                          \
    /* members that share part of their state: the ensemble entry's arguments + (shared_mask, eta_member_stride) */            \
    int32_t cloudsc2_tl_enss_##SFX(CS2_TL_ARGS(T), void* stream, CS2_ENSS_ARGS) {                                              \
        CS2_TL_CALL(T, cs2::kEns | cs2::kShared);                                                                              \
        CS2_ENSS;                                                                                                              \
        return tl_masked_impl<T>("cloudsc2_tl_enss_" #SFX, c);                                                                 \
    }                                                                                                                          \
    int32_t cloudsc2_tl_step_enss_##SFX(CS2_TL_ARGS(T), void* stream, CS2_ENSS_ARGS) {                                         \
        CS2_TL_CALL(T, cs2::kStep | cs2::kEns | cs2::kShared);                                                                 \
        CS2_ENSS;                                                                                                              \
        return tl_masked_impl<T>("cloudsc2_tl_step_enss_" #SFX, c);                                                            \
    }                                                                                                                          \
    int32_t cloudsc2_ad_enss_##SFX(CS2_AD_ARGS(T), void* stream, CS2_ENSS_ARGS) {                                              \
        CS2_AD_CALL(T, cs2::kEns | cs2::kShared);                                                                              \
        CS2_ENSS;                                                                                                              \
        return ad_masked_impl<T>("cloudsc2_ad_enss_" #SFX, c);                                                                 \
    }                                                                                                                          \
    int32_t cloudsc2_ad_step_enss_##SFX(CS2_AD_ARGS(T), void* stream, CS2_ENSS_ARGS) {                                         \
        CS2_AD_CALL(T, cs2::kStep | cs2::kEns | cs2::kShared);                                                                 \
        CS2_ENSS;                                                                                                              \
        return ad_masked_impl<T>("cloudsc2_ad_step_enss_" #SFX, c);                                                            \
    }                                                                                                                          \
    /* members times directions: the multi entry's arguments + (nmem, member_stride, in_member_stride, out_member_stride) */   \
    int32_t cloudsc2_ad_multi_ens_##SFX(CS2_AD_ARGS(T), void* stream, CS2_DIRS_ARGS, CS2_MENS_ARGS) {                          \
        CS2_AD_CALL(T, cs2::kMulti | cs2::kEns);                                                                               \
        CS2_DIRS; CS2_MENS;                                                                                                    \
        return ad_masked_impl<T>("cloudsc2_ad_multi_ens_" #SFX, c);                                                            \
    }                                                                                                                          \
    int32_t cloudsc2_ad_multi_step_ens_##SFX(CS2_AD_ARGS(T), void* stream, CS2_DIRS_ARGS, CS2_MENS_ARGS) {                     \
        CS2_AD_CALL(T, cs2::kStep | cs2::kMulti | cs2::kEns);                                                                  \
        CS2_DIRS; CS2_MENS;                                                                                                    \
        return ad_masked_impl<T>("cloudsc2_ad_multi_step_ens_" #SFX, c);                                                       \
    }                                                                                                                          \
    /* the trajectory adjoints with the evaporation block: + (cover, cover_ready), in front of `stream` in the single */       \
    /* entries and their ensemble forms, behind the directions in the multi entries */                                         \
    int32_t cloudsc2_ad_evap_##SFX(CS2_AD_ARGS(T), CS2_COVER_ARGS(T), void* stream) {                                          \
        CS2_AD_CALL(T, cs2::kEvap);                                                                                            \
        CS2_COVER;                                                                                                             \
        return ad_masked_impl<T>("cloudsc2_ad_evap_" #SFX, c);                                                                 \
    }                                                                                                                          \
    int32_t cloudsc2_ad_evap_step_##SFX(CS2_AD_ARGS(T), CS2_COVER_ARGS(T), void* stream) {                                     \
        CS2_AD_CALL(T, cs2::kStep | cs2::kEvap);                                                                               \
        CS2_COVER;                                                                                                             \
        return ad_masked_impl<T>("cloudsc2_ad_evap_step_" #SFX, c);                                                            \
    }                                                                                                                          \
    int32_t cloudsc2_ad_evap_multi_##SFX(CS2_AD_ARGS(T), void* stream, CS2_DIRS_ARGS, CS2_COVER_ARGS(T)) {                     \
        CS2_AD_CALL(T, cs2::kMulti | cs2::kEvap);                                                                              \
        CS2_DIRS; CS2_COVER;                                                                                                   \
        return ad_masked_impl<T>("cloudsc2_ad_evap_multi_" #SFX, c);                                                           \
    }                                                                                                                          \
    int32_t cloudsc2_ad_evap_multi_step_##SFX(CS2_AD_ARGS(T), void* stream, CS2_DIRS_ARGS, CS2_COVER_ARGS(T)) {                \
        CS2_AD_CALL(T, cs2::kStep | cs2::kMulti | cs2::kEvap);                                                                 \
        CS2_DIRS; CS2_COVER;                                                                                                   \
        return ad_masked_impl<T>("cloudsc2_ad_evap_multi_step_" #SFX, c);                                                      \
    }                                                                                                                          \
    int32_t cloudsc2_ad_evap_ens_##SFX(CS2_AD_ARGS(T), CS2_COVER_ARGS(T), void* stream, CS2_ENS_ARGS) {                        \
        CS2_AD_CALL(T, cs2::kEns | cs2::kEvap);                                                                                \
        CS2_ENS; CS2_COVER;                                                                                                    \
        return ad_masked_impl<T>("cloudsc2_ad_evap_ens_" #SFX, c);                                                             \
    }                                                                                                                          \
    int32_t cloudsc2_ad_evap_step_ens_##SFX(CS2_AD_ARGS(T), CS2_COVER_ARGS(T), void* stream, CS2_ENS_ARGS) {                   \
        CS2_AD_CALL(T, cs2::kStep | cs2::kEns | cs2::kEvap);                                                                   \
        CS2_ENS; CS2_COVER;                                                                                                    \
        return ad_masked_impl<T>("cloudsc2_ad_evap_step_ens_" #SFX, c);                                                        \
    }                                                                                                                          \
    /* the ensemble forms of the two NL entries: the single entry's arguments + (nmem, member_stride) */                       \
    int32_t cloudsc2_nl_ens_##SFX(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const T* const* in,             \
                                  const T* eta, T* const* out, double dt, void* stream, CS2_ENS_ARGS) {                        \
        return nl_impl<T>("cloudsc2_nl_ens_" #SFX, p, nx, nz, ls, in, eta, out, dt, stream, true, {nmem, ms});                 \
    }                                                                                                                          \
    int32_t cloudsc2_nl_fused_ens_##SFX(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const T* const* in,       \
                                        const T* const* in_i, double pf, T* qsat_out, const T* eta, T* const* out, double dt,  \
                                        void* stream, CS2_ENS_ARGS) {                                                          \
        return nl_fused_impl<T>("cloudsc2_nl_fused_ens_" #SFX, p, nx, nz, ls, in, in_i, pf, qsat_out, eta, out, dt, stream,    \
                                true, {nmem, ms});                                                                             \
    }                                                                                                                          \
    /* ... and their shared-state forms: + (shared_mask, eta_member_stride) */                                                 \
    int32_t cloudsc2_nl_enss_##SFX(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const T* const* in,            \
                                   const T* eta, T* const* out, double dt, void* stream, CS2_ENSS_ARGS) {                      \
        return nl_impl<T>("cloudsc2_nl_enss_" #SFX, p, nx, nz, ls, in, eta, out, dt, stream, true, CS2_ENSS_MEMBERS, true);    \
    }                                                                                                                          \
    int32_t cloudsc2_nl_fused_enss_##SFX(const Cloudsc2Params* p, int32_t nx, int32_t nz, int64_t ls, const T* const* in,      \
                                         const T* const* in_i, double pf, T* qsat_out, const T* eta, T* const* out, double dt, \
                                         void* stream, CS2_ENSS_ARGS) {                                                        \
        return nl_fused_impl<T>("cloudsc2_nl_fused_enss_" #SFX, p, nx, nz, ls, in, in_i, pf, qsat_out, eta, out, dt, stream,   \
                                true, CS2_ENSS_MEMBERS, true);                                                                 \
    }
CS2_MASKED_ENTRIES(f64, double)
CS2_MASKED_ENTRIES(f32, float)
#undef CS2_MASKED_ENTRIES
#undef CS2_TL_ARGS
#undef CS2_AD_ARGS
#undef CS2_DIRS_ARGS
#undef CS2_ENS_ARGS
#undef CS2_MENS_ARGS
#undef CS2_COVER_ARGS
#undef CS2_TL_CALL
#undef CS2_AD_CALL
#undef CS2_DIRS
#undef CS2_ENS
#undef CS2_MENS
#undef CS2_ENSS
#undef CS2_ENSS_MEMBERS
#undef CS2_ENSS_ARGS
#undef CS2_COVER

}  // extern "C"
