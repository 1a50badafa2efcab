// rbsensor_probes.hip -- value-by-value probes of the per-pixel likelihood's device code.  TEST BUILD ONLY: rbsensor_capi.hip
// includes this file under RBS_TEST_HOOKS (librbsensor_mi355x_hooks.so, `make hooks`); the release library has none of it.
//
// Under __HIP_DEVICE_COMPILE__ rbs_math.h takes branches that no host build compiles (the Horner literals of exp_nonpos, the
// hex-coded constants and the classf test of log_f32, the reciprocal expansions div_f32 / rcp_f64, ocml exp / sqrt in
// frame_terms, the LDS copy of the tables), and the F32 pixel model exists on the device only.  Each probe runs ONE of those
// inline functions -- the function the raster kernels call, nothing copied -- over a host array, one thread per element, and
// hands every value back: tests/test_gpu_pixel_math.py compares them one by one.
//
// Entry points (rbs_test_*): host arrays in, host arrays out, synchronous on the current device.  Null pointers and n < 0 (or
// n > kProbeMax) are RBS_ERR_INVALID_ARGUMENT, n == 0 is RBS_OK and touches nothing, a HIP failure is RBS_ERR_HIP.
namespace rbs {
namespace probe {

constexpr int64_t kProbeMax = int64_t(1) << 26;   // elements per call (the largest buffer, [n][4] doubles, is then 2 GB)
constexpr int kProbeTabErfc = rbsm::kErfcIntervals * rbsm::kErfcCoefs, kProbeTabLog = rbsm::kLogIntervals * 2;
static_assert(!RBS_MATH_LDS || kMathTabDoubles == kProbeTabErfc + kProbeTabLog, "the probes' LDS copy is the raster kernel's");

__device__ inline size_t probe_index() { return (size_t)blockIdx.x * blockDim.x + threadIdx.x; }

// The tables as the raster kernel's evaluation sees them.  LDS: the block's copy, filled by the raster kernel's own two loops
// (blocks of kBlock threads) and handed out as `tab` and `tab + ne`, as MathTabs is built there; else the constant tables.
// Every thread of the block calls this (it ends in a barrier).
template <bool LDS>
__device__ inline MathTabs probe_tabs(double* tab)
{
    if (!LDS) return MathTabs{rbsm::kErfcTab, rbsm::kLogTab, nullptr};
    constexpr int ne = kProbeTabErfc, nl = kProbeTabLog;
    for (int i = threadIdx.x; i < ne; i += kBlock) tab[i] = rbsm::kErfcTab[i];
    for (int i = threadIdx.x; i < nl; i += kBlock) tab[ne + i] = rbsm::kLogTab[i];
    __syncthreads();
    return MathTabs{tab, tab + ne, nullptr};
}

__global__ void __launch_bounds__(kBlock) exp_nonpos_kernel(const double* __restrict__ x, double* __restrict__ out, size_t n)
{
    const size_t i = probe_index();
    if (i < n) out[i] = rbsm::exp_nonpos(x[i], rbsm::kExpPoly);
}

template <bool LDS>
__global__ void __launch_bounds__(kBlock) erfc_pos_kernel(const double* __restrict__ z, double* __restrict__ out, size_t n)
{
    __shared__ alignas(16) double tab[kProbeTabErfc + kProbeTabLog];
    const MathTabs M = probe_tabs<LDS>(tab);
    const size_t i = probe_index();
    if (i < n) out[i] = rbsm::erfc_pos(z[i], M.erfc);
}

template <bool LDS>
__global__ void __launch_bounds__(kBlock) log_f32_kernel(const float* __restrict__ x, double* __restrict__ out, size_t n)
{
    __shared__ alignas(16) double tab[kProbeTabErfc + kProbeTabLog];
    const MathTabs M = probe_tabs<LDS>(tab);
    const size_t i = probe_index();
    if (i < n) out[i] = rbsm::log_f32(x[i], M.logt);
}

__global__ void __launch_bounds__(kBlock) div_f32_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, size_t n)
{
    const size_t i = probe_index();
    if (i < n) out[i] = rbsm::div_f32(a[i], b[i]);
}

__global__ void __launch_bounds__(kBlock) rcp_f64_kernel(const double* __restrict__ x, double* __restrict__ out, size_t n)
{
    const size_t i = probe_index();
    if (i < n) out[i] = rbsm::rcp_f64(x[i]);
}

// The F64 pixel term as the raster kernel's batch evaluates it: pixel_loglik<false> on the aux entry frame_aux_kernel stored
// (P.aux, pixel i), the tables in LDS.
__global__ void __launch_bounds__(kBlock) pixel_f64_kernel(const DevParams P, const float* __restrict__ depth, const float* __restrict__ prior,
                                                           double* __restrict__ term, float* __restrict__ post, size_t n)
{
    __shared__ alignas(16) double tab[kProbeTabErfc + kProbeTabLog];
    const MathTabs M = probe_tabs<RBS_MATH_LDS != 0>(tab);
    const size_t i = probe_index();
    if (i < n) {
        float q;
        term[i] = pixel_loglik<false>(P, M, (int)i, depth[i], prior[i], q);
        post[i] = q;
    }
}

__global__ void __launch_bounds__(kBlock) pixel_f32_kernel(const DevParams P, const float* __restrict__ obs, const float* __restrict__ depth,
                                                           const float* __restrict__ prior, double* __restrict__ term, float* __restrict__ post, size_t n)
{
    const size_t i = probe_index();
    if (i < n) {
        float q;
        term[i] = pixel_loglik_f32(P, depth[i], prior[i], obs[i], q);
        post[i] = q;
    }
}

// Device buffers of one call: freed on every way out.
struct Buffers {
    void* p[8] = {};
    int k = 0;
    hipError_t err = hipSuccess;
    template <class T> T* make(size_t count, const T* from = nullptr)
    {
        void* d = nullptr;
        if (err == hipSuccess) err = hipMalloc(&d, sizeof(T) * count);
        if (err != hipSuccess) return nullptr;
        p[k++] = d;
        if (from) err = hipMemcpy(d, from, sizeof(T) * count, hipMemcpyHostToDevice);
        return static_cast<T*>(d);
    }
    template <class T> void fetch(T* to, const T* d, size_t count)
    {
        if (err == hipSuccess) err = hipMemcpy(to, d, sizeof(T) * count, hipMemcpyDeviceToHost);
    }
    // after a launch: its launch error, then the kernel's own
    void ran()
    {
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
    }
    int32_t status() const { return err == hipSuccess ? RBS_OK : RBS_ERR_HIP; }
    ~Buffers() { for (int i = 0; i < k; ++i) (void)hipFree(p[i]); }
};

inline dim3 probe_grid(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }
inline bool probe_refused(int64_t n) { return n < 0 || n > kProbeMax; }

// the model parameters the pixel terms read, as rbs_create derives them
inline DevParams probe_params(double tw, double ms, double sf, double lam)
{
    DevParams P{};
    P.tw = tw; P.ms = ms; P.sf = sf; P.lambda = lam;
    P.cv0 = (1.0 - tw) / std::sqrt(M_PI);
    return P;
}

}  // namespace probe
}  // namespace rbs

extern "C" {

int32_t rbs_test_exp_nonpos(const double* x, double* out, int64_t n)
{
    namespace pr = rbs::probe;
    if (!x || !out || pr::probe_refused(n)) return RBS_ERR_INVALID_ARGUMENT;
    if (n == 0) return RBS_OK;
    pr::Buffers B;
    const double* dx = B.make<double>(n, x);
    double* dout = B.make<double>(n);
    if (B.err == hipSuccess) { hipLaunchKernelGGL(pr::exp_nonpos_kernel, pr::probe_grid(n), dim3(rbs::kBlock), 0, 0, dx, dout, (size_t)n); B.ran(); }
    B.fetch(out, dout, n);
    return B.status();
}

int32_t rbs_test_erfc_pos(const double* z, double* out, int64_t n, int32_t lds_tables)
{
    namespace pr = rbs::probe;
    if (!z || !out || pr::probe_refused(n)) return RBS_ERR_INVALID_ARGUMENT;
    if (n == 0) return RBS_OK;
    pr::Buffers B;
    const double* dz = B.make<double>(n, z);
    double* dout = B.make<double>(n);
    if (B.err == hipSuccess) {
        if (lds_tables) hipLaunchKernelGGL(pr::erfc_pos_kernel<true>, pr::probe_grid(n), dim3(rbs::kBlock), 0, 0, dz, dout, (size_t)n);
        else hipLaunchKernelGGL(pr::erfc_pos_kernel<false>, pr::probe_grid(n), dim3(rbs::kBlock), 0, 0, dz, dout, (size_t)n);
        B.ran();
    }
    B.fetch(out, dout, n);
    return B.status();
}

int32_t rbs_test_log_f32(const float* x, double* out, int64_t n, int32_t lds_tables)
{
    namespace pr = rbs::probe;
    if (!x || !out || pr::probe_refused(n)) return RBS_ERR_INVALID_ARGUMENT;
    if (n == 0) return RBS_OK;
    pr::Buffers B;
    const float* dx = B.make<float>(n, x);
    double* dout = B.make<double>(n);
    if (B.err == hipSuccess) {
        if (lds_tables) hipLaunchKernelGGL(pr::log_f32_kernel<true>, pr::probe_grid(n), dim3(rbs::kBlock), 0, 0, dx, dout, (size_t)n);
        else hipLaunchKernelGGL(pr::log_f32_kernel<false>, pr::probe_grid(n), dim3(rbs::kBlock), 0, 0, dx, dout, (size_t)n);
        B.ran();
    }
    B.fetch(out, dout, n);
    return B.status();
}

int32_t rbs_test_div_f32(const float* a, const float* b, float* out, int64_t n)
{
    namespace pr = rbs::probe;
    if (!a || !b || !out || pr::probe_refused(n)) return RBS_ERR_INVALID_ARGUMENT;
    if (n == 0) return RBS_OK;
    pr::Buffers B;
    const float* da = B.make<float>(n, a);
    const float* db = B.make<float>(n, b);
    float* dout = B.make<float>(n);
    if (B.err == hipSuccess) { hipLaunchKernelGGL(pr::div_f32_kernel, pr::probe_grid(n), dim3(rbs::kBlock), 0, 0, da, db, dout, (size_t)n); B.ran(); }
    B.fetch(out, dout, n);
    return B.status();
}

int32_t rbs_test_rcp_f64(const double* x, double* out, int64_t n)
{
    namespace pr = rbs::probe;
    if (!x || !out || pr::probe_refused(n)) return RBS_ERR_INVALID_ARGUMENT;
    if (n == 0) return RBS_OK;
    pr::Buffers B;
    const double* dx = B.make<double>(n, x);
    double* dout = B.make<double>(n);
    if (B.err == hipSuccess) { hipLaunchKernelGGL(pr::rcp_f64_kernel, pr::probe_grid(n), dim3(rbs::kBlock), 0, 0, dx, dout, (size_t)n); B.ran(); }
    B.fetch(out, dout, n);
    return B.status();
}

// out4: [n][4], the aux entries {1/(sqrt2 sigma), k, o, e_o} as frame_aux_kernel (frame_aux_pixel) stores them
int32_t rbs_test_frame_terms(const float* obs, int64_t n, double tw, double ms, double sf, double lam, double* out4)
{
    namespace pr = rbs::probe;
    if (!obs || !out4 || pr::probe_refused(n)) return RBS_ERR_INVALID_ARGUMENT;
    if (n == 0) return RBS_OK;
    pr::Buffers B;
    const float* dobs = B.make<float>(n, obs);
    double* daux = B.make<double>(4 * (size_t)n);
    if (B.err == hipSuccess) {
        hipLaunchKernelGGL(rbs::frame_aux_kernel, pr::probe_grid(n), dim3(rbs::kBlock), 0, 0, dobs, daux, (float*)nullptr, (int)n, tw, ms, sf, lam,
                           (float*)nullptr);
        B.ran();
    }
    B.fetch(out4, daux, 4 * (size_t)n);
    return B.status();
}

// term[n], posterior[n] of (observation, rendered depth, prior)[n] in likelihood precision F64: frame_aux_kernel, then
// pixel_loglik<false> on the stored entries
int32_t rbs_test_pixel_f64(const float* obs, const float* depth, const float* prior, int64_t n, double tw, double ms, double sf, double lam,
                           double* term, float* posterior)
{
    namespace pr = rbs::probe;
    if (!obs || !depth || !prior || !term || !posterior || pr::probe_refused(n)) return RBS_ERR_INVALID_ARGUMENT;
    if (n == 0) return RBS_OK;
    pr::Buffers B;
    const float* dobs = B.make<float>(n, obs);
    const float* ddepth = B.make<float>(n, depth);
    const float* dprior = B.make<float>(n, prior);
    double* daux = B.make<double>(4 * (size_t)n);
    double* dterm = B.make<double>(n);
    float* dpost = B.make<float>(n);
    if (B.err == hipSuccess) {
        DevParams P = pr::probe_params(tw, ms, sf, lam);
        P.npx = (int)n;
        P.aux = daux;
        hipLaunchKernelGGL(rbs::frame_aux_kernel, pr::probe_grid(n), dim3(rbs::kBlock), 0, 0, dobs, daux, (float*)nullptr, (int)n, tw, ms, sf, lam,
                           (float*)nullptr);
        hipLaunchKernelGGL(pr::pixel_f64_kernel, pr::probe_grid(n), dim3(rbs::kBlock), 0, 0, P, ddepth, dprior, dterm, dpost, (size_t)n);
        B.ran();
    }
    B.fetch(term, dterm, n);
    B.fetch(posterior, dpost, n);
    return B.status();
}

// ... in likelihood precision F32: pixel_loglik_f32
int32_t rbs_test_pixel_f32(const float* obs, const float* depth, const float* prior, int64_t n, double tw, double ms, double sf, double lam,
                           double* term, float* posterior)
{
    namespace pr = rbs::probe;
    if (!obs || !depth || !prior || !term || !posterior || pr::probe_refused(n)) return RBS_ERR_INVALID_ARGUMENT;
    if (n == 0) return RBS_OK;
    pr::Buffers B;
    const float* dobs = B.make<float>(n, obs);
    const float* ddepth = B.make<float>(n, depth);
    const float* dprior = B.make<float>(n, prior);
    double* dterm = B.make<double>(n);
    float* dpost = B.make<float>(n);
    if (B.err == hipSuccess) {
        const DevParams P = pr::probe_params(tw, ms, sf, lam);
        hipLaunchKernelGGL(pr::pixel_f32_kernel, pr::probe_grid(n), dim3(rbs::kBlock), 0, 0, P, dobs, ddepth, dprior, dterm, dpost, (size_t)n);
        B.ran();
    }
    B.fetch(term, dterm, n);
    B.fetch(posterior, dpost, n);
    return B.status();
}

}  // extern "C"
