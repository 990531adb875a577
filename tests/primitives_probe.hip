// Test-only probe of the arithmetic primitives in csrc/cloudsc2_common.hpp (tests/test_math_primitives.py).
//
// Every launcher is elementwise: one thread per element, plain global loads and stores, bounds-checked, launched on the
// null stream and synchronised before it returns (0 on success, the hipError_t otherwise).  Each kernel calls the very
// function the level loops call - nothing is restated here - and writes, where there is one, the compiler's or ocml's
// version of the same operation beside it.  Built by the test into a temporary directory; never linked into
// libcloudsc2_hip.so.
#include "cloudsc2_common.hpp"

namespace {

using cs2::ExpK;
using cs2::Ext;

constexpr int kBlock = 256;

__device__ __forceinline__ int64_t gid() { return int64_t(blockIdx.x) * kBlock + threadIdx.x; }

template <typename T>
__global__ void frcp_kernel(const T* x, T* out, T* out_div, int64_t n) {
    const int64_t i = gid();
    if (i >= n) return;
    out[i] = cs2::frcp<T>(x[i]);
    out_div[i] = T(1.0) / x[i];
}

template <typename T>
__global__ void fexp_kernel(ExpK<T> xk, const T* x, T* out, T* out_ocml, int64_t n) {
    const int64_t i = gid();
    if (i >= n) return;
    out[i] = cs2::fexp<T>(xk, x[i]);
    out_ocml[i] = cs2::rexp<T>(x[i]);
}

template <typename T>
__global__ void foealf_kernel(Ext<T> e, const T* t, T* out_alfa, T* out_alfcu, int64_t n) {
    const int64_t i = gid();
    if (i >= n) return;
    out_alfa[i] = cs2::foealfa<T>(e, t[i]);
    out_alfcu[i] = cs2::foealfcu<T>(e, t[i]);
}

template <typename T, int MODE>
__global__ void saturation_kernel(Ext<T> e, ExpK<T> xk, const T* t, const T* ap, T* out, int64_t n) {
    const int64_t i = gid();
    if (i >= n) return;
    out[i] = cs2::saturation_point<T, MODE>(e, xk, t[i], ap[i]);
}

template <typename T>
__global__ void minmax_kernel(const T* a, const T* b, T* out_min, T* out_max, int64_t n) {
    const int64_t i = gid();
    if (i >= n) return;
    out_min[i] = cs2::rmin<T>(a[i], b[i]);
    out_max[i] = cs2::rmax<T>(a[i], b[i]);
}

// out = rounded_product(f, x) - y: exactly 0 for y = fl(f x) when the product is rounded before the subtraction, and the
// rounding residual f x - fl(f x) if it were contracted into an fma - which `out_fused` spells out for comparison.
template <typename T>
__global__ void rounded_product_kernel(const T* f, const T* x, const T* y, T* out, T* out_fused, int64_t n) {
    const int64_t i = gid();
    if (i >= n) return;
    out[i] = cs2::rounded_product<T>(f[i], x[i]) - y[i];
    out_fused[i] = __builtin_fma(f[i], x[i], -y[i]);
}

template <typename T>
__global__ void logistic_kernel(ExpK<T> xk, T fw2, T rlptrc, const T* t, T* out_fwat, T* out_fwat_nl, T* out_sech2,
                                int64_t n) {
    const int64_t i = gid();
    if (i >= n) return;
    T ex, rr;
    out_fwat[i] = cs2::logistic_fwat<T>(xk, fw2, rlptrc, t[i], ex, rr);     // cloudsc2_tl, cloudsc2_ad
    out_fwat_nl[i] = cs2::logistic_fwat<T>(xk, fw2, rlptrc, t[i]);          // cloudsc2_nl
    out_sech2[i] = cs2::logistic_sech2<T>(ex, rr);
}

template <typename K, typename... A>
int launch(K kernel, int64_t n, A... args) {
    if (n < 0 || n > (int64_t(1) << 31)) return -1;
    if (n == 0) return 0;
    const unsigned grid = unsigned((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, nullptr, args..., n);
    hipError_t rc = hipGetLastError();
    if (rc == hipSuccess) rc = hipStreamSynchronize(nullptr);
    return int(rc);
}

}  // namespace

#define PROBE_BOTH(DECL) DECL(f64, double) DECL(f32, float)

extern "C" {

#define PROBE_FRCP(S, T) \
    int probe_frcp_##S(const T* x, T* out, T* out_div, int64_t n) { return launch(frcp_kernel<T>, n, x, out, out_div); }
PROBE_BOTH(PROBE_FRCP)

#define PROBE_FEXP(S, T)                                                             \
    int probe_fexp_##S(const T* x, T* out, T* out_ocml, int64_t n) {                 \
        return launch(fexp_kernel<T>, n, cs2::make_expk<T>(), x, out, out_ocml);     \
    }
PROBE_BOTH(PROBE_FEXP)

#define PROBE_FOEALF(S, T)                                                                          \
    int probe_foealf_##S(const Cloudsc2Params* p, const T* t, T* out_alfa, T* out_alfcu, int64_t n) {  \
        return launch(foealf_kernel<T>, n, cs2::make_ext<T>(*p), t, out_alfa, out_alfcu);            \
    }
PROBE_BOTH(PROBE_FOEALF)

// mode 0: LPHYLIN; 1: KFLAG == 1 (f_foeewmcu); 2: f_foeewm - the MODE of cs2::saturation_point
#define PROBE_SATURATION(S, T)                                                                            \
    int probe_saturation_##S(const Cloudsc2Params* p, int mode, const T* t, const T* ap, T* out, int64_t n) { \
        const Ext<T> e = cs2::make_ext<T>(*p);                                                            \
        const ExpK<T> xk = cs2::make_expk<T>();                                                           \
        if (mode == 0) return launch(saturation_kernel<T, 0>, n, e, xk, t, ap, out);                      \
        if (mode == 1) return launch(saturation_kernel<T, 1>, n, e, xk, t, ap, out);                      \
        if (mode == 2) return launch(saturation_kernel<T, 2>, n, e, xk, t, ap, out);                      \
        return -1;                                                                                        \
    }
PROBE_BOTH(PROBE_SATURATION)

#define PROBE_MINMAX(S, T)                                                         \
    int probe_minmax_##S(const T* a, const T* b, T* out_min, T* out_max, int64_t n) { \
        return launch(minmax_kernel<T>, n, a, b, out_min, out_max);                \
    }
PROBE_BOTH(PROBE_MINMAX)

#define PROBE_ROUNDED_PRODUCT(S, T)                                                                      \
    int probe_rounded_product_##S(const T* f, const T* x, const T* y, T* out, T* out_fused, int64_t n) { \
        return launch(rounded_product_kernel<T>, n, f, x, y, out, out_fused);                            \
    }
PROBE_BOTH(PROBE_ROUNDED_PRODUCT)

// fw2 is the launchers' own constant (make_nlk: 2 * 0.17 in the working precision), RLPTRC the external
#define PROBE_LOGISTIC(S, T)                                                                                          \
    int probe_logistic_##S(const Cloudsc2Params* p, const T* t, T* out_fwat, T* out_fwat_nl, T* out_sech2, int64_t n) { \
        const T fw2 = cs2::make_nlk<T>(*p, 1.0, false).fw2;                                                           \
        return launch(logistic_kernel<T>, n, cs2::make_expk<T>(), fw2, cs2::make_ext<T>(*p).RLPTRC, t, out_fwat,       \
                      out_fwat_nl, out_sech2);                                                                        \
    }
PROBE_BOTH(PROBE_LOGISTIC)

}  // extern "C"
