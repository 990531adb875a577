// Host side: THE declarations of the launchers (cs2::launch_*), shared by the C boundary (cloudsc2_capi.hip) and the units that
// define them, and the call descriptor of the masked TL / AD family.  A definition that drifts from its declaration here no
// longer matches its explicit instantiation: a compile error in its own unit.
#pragma once

#include "cloudsc2_common.hpp"

namespace cs2 {

// ---- the masked family (cloudsc2_{tl,ad}_{masked,step,multi,multi_step,ens,step_ens}_*, cloudsc2_ad_multi{,_step}_ens_*,
// cloudsc2_ad_evap_*): one call descriptor from the extern "C" wrapper through the checks to the launcher.
// What the ENTRY is, not what its arguments hold: a multi entry called with ndir = 0, an ensemble entry called with
// nmem = 0 keep their bit (and are refused by the checks); an entry without the bit leaves its group zero.
enum CallForm : unsigned {
    kMasked = 0u,  // the plain masked entry: none of the below
    kStep = 1u,    // `saturation` fused in (the *_step_* entries)
    kMulti = 2u,   // has the directions group
    kEns = 4u,     // has the members group
    kEvap = 8u,    // has the cover group: the adjoints WITH the evaporation block
    kShared = 16u, // with kEns: the *_enss_* entries - the members group carries shared_mask and eta_ms too
};
struct CallDirs {      // direction d of a field lies d * in_ds (inputs) / d * out_ds (outputs) elements behind direction 0
    int ndir;
    int64_t in_ds, out_ds;
};
struct CallMembers {   // member m of every field lies m * ms elements behind member 0
    int nmem;
    int64_t ms;
    // kMulti and kEns (cloudsc2_ad_multi_ens_* / _multi_step_ens_*): `ms` is the state's and the trajectory fluxes'; member m of
    // a batched forcing / adjoint lies m * in_ms / m * out_ms elements behind member 0 (its directions inside the member)
    int64_t in_ms, out_ms;
    // kShared (cloudsc2_*_enss_*): bit i of shared_mask - state input i is ONE field read by every member; the two
    // CLOUDSC2_ENSS_*_MAJOR bits choose the block order of the launch; eta_ms: 0, or the member stride of `eta` (elements)
    int64_t shared_mask, eta_ms;
};
// the kernels' geometry of a kShared call (the checks have passed); bpm: column blocks per member
inline EnssGeom enss_geom(const CallMembers& m, int bpm) {
    const int order = (m.shared_mask & CLOUDSC2_ENSS_COLUMN_MAJOR) ? kColumnMajor
                      : (m.shared_mask & CLOUDSC2_ENSS_MEMBER_MAJOR) ? kMemberMajor : kEnssDefaultOrder;
    return EnssGeom{{m.ms, bpm}, uint32_t(m.shared_mask & 0xFFFF), m.nmem, order, m.eta_ms};
}
template <typename T>
struct CallCover {     // the caller's precipitation-cover field; cover_ready: it already holds the forward sweep's values
    T* cover;
    int cover_ready;
};
template <typename T>
struct CallHead {
    const Cloudsc2Params* p;
    int nx, nz;
    int64_t ls;
    const T* const* in;
    const T* zero;     // the zero line: what a NULL entry of in_i / in_adj reads
    const T* eta;
    double dt;
    hipStream_t stream;
    unsigned form;     // CallForm bits
    bool is(CallForm f) const { return (form & f) != 0; }
};
template <typename T>
struct TLCall : CallHead<T> {
    const T* const* in_i;
    T* const* out;
    T* const* out_i;
    CallDirs dirs;
    CallMembers members;
};
template <typename T>
struct ADCall : CallHead<T> {
    const T* const* in_adj;
    const T *traj_l, *traj_n;
    T* const* out_adj;
    CallDirs dirs;
    CallMembers members;
    CallCover<T> cover;
};

template <typename T>
int launch_tl_masked(const TLCall<T>&);
template <typename T>
int launch_tl_dirs(const TLCall<T>&);
template <typename T>
int launch_ad_masked(const ADCall<T>&);
template <typename T>
int launch_ad_dirs(const ADCall<T>&);
template <typename T>
int launch_ad_cover(const ADCall<T>&);

// ---- the plain stencils, the ensemble NL form and the aux kernels: positional, as their C entries are
template <typename T>
int launch_nl(const Cloudsc2Params&, int, int, int64_t, const T* const*, const T*, T* const*, double, hipStream_t,
              const T* const*, double, T*, double*);
template <typename T>
int launch_nl_ens(const Cloudsc2Params&, int, int, int64_t, const T* const*, const T*, T* const*, double, hipStream_t, T*,
                  const CallMembers&, bool shared);
template <typename T>
int launch_nl_taylor_multi(const Cloudsc2Params&, int, int, int64_t, const T* const*, const T* const*, int, const double*,
                           const T*, const T* const*, double*, double, hipStream_t, double);
template <typename T>
int launch_tl(const Cloudsc2Params&, int, int, int64_t, const T* const*, const T* const*, const T*, T* const*,
              T* const*, double, hipStream_t, double);
template <typename T>
int launch_ad(const Cloudsc2Params&, int, int, int64_t, const T* const*, const T* const*, const T*, T* const*,
              T* const*, double, hipStream_t, const T* traj_l, const T* traj_n);
template <typename T>
int launch_saturation(const Cloudsc2Params&, int, int, int64_t, const T*, const T*, T*, hipStream_t);
template <typename T>
int launch_saturation_tl(const Cloudsc2Params&, int, int, int64_t, const T*, const T*, const T*, const T*, T*, T*,
                         hipStream_t);
template <typename T>
int launch_saturation_ad(const Cloudsc2Params&, int, int, int64_t, const T*, const T*, const T*, T*, T*, int, hipStream_t);
template <typename T>
int launch_increment(const Cloudsc2Params&, int, int, int64_t, const T* const*, T* const*, double, hipStream_t);
template <typename T>
int launch_perturb(int, int, int64_t, const T* const*, const T* const*, T* const*, double, hipStream_t);
int field_sums_blocks(int, int);
int column_dots_chunks(int);
template <typename T>
int launch_field_sums(int, int, int64_t, int, const T* const*, const T* const*, double*, hipStream_t);
template <typename T>
int launch_column_dots(int, int, int64_t, int, const T* const*, const T* const*, double*, int, hipStream_t);

}  // namespace cs2
