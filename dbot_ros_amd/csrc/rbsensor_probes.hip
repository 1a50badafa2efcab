// rbsensor_probes.hip -- value-by-value probes of the per-pixel likelihood's device code.  TEST BUILD ONLY: rbsensor_capi.hip
// includes this file under RBS_TEST_HOOKS (librbsensor_mi355x_hooks.so, `make hooks`); the release library has none of it.
//
// Under __HIP_DEVICE_COMPILE__ rbs_math.h takes branches that no host build compiles (the Horner literals of exp_nonpos, the
// hex-coded constants and the classf test of log_f32, the reciprocal expansions div_f32 / rcp_f64, ocml exp / sqrt in
// frame_terms, the LDS copy of the tables), and the F32 pixel model exists on the device only.  Each probe runs ONE of those
// inline functions -- the function the raster kernels call, nothing copied -- over a host array, one thread per element, and
// hands every value back: tests/test_gpu_pixel_math.py compares them one by one.
//
// rbs_test_filter does the same for the particle filter's kernels (rbsensor_tracker.hip): it builds an rbt::TrackerDev from host
// arrays, launches a caller-chosen order of the frame's steps through the launch_* helpers rbs_tracker_submit itself uses
// (rbsensor_capi.hip: no kernel body and no launch geometry is restated here), and hands every array back:
// tests/test_gpu_filter_kernels.py.
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
    static constexpr int kMax = 32;
    void* p[kMax] = {};
    int k = 0;
    hipError_t err = hipSuccess;
    template <class T> T* make(size_t count, const T* from = nullptr)
    {
        void* d = nullptr;
        if (err == hipSuccess && k >= kMax) err = hipErrorOutOfMemory;
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

// ---------------------------------------------------------------------------- the particle filter's kernels
// One call's arrays.  Every array is copied to the device before the first step and back after the last one, under the name
// it has THEN (RBS_TEST_STEP_SWAP exchanges an array with its gather target, as rbs_tracker_submit does after a sampling
// block), so the caller sees everything the kernels wrote and, by the values it put there, everything they left alone.
// normals [parts][n][6] and uniforms [parts][n] may be null: the device generator then draws them from (seed, frame).
struct rbs_test_filter_io {
    int32_t n, parts;
    double sigma[6];
    double vf, max_kl;
    uint64_t seed, frame;
    double* part_old; double* part_new; double* part_old2; double* part_new2;   // [n][parts * 12]
    double* noise; double* noise2;                                                // [n][parts][6]
    double* logw; double* ll; double* ll2; double* ll_new; double* cdf;          // [n]
    int32_t* idx; int32_t* idx2; int32_t* parents;                               // [n]
    double* deflt;                                                                // [parts * 12]
    double* mean;                                                                 // [parts * 12 + parts * 9]
    double* poses;                                                                // [n][parts][12]
    int32_t* flag;                                                                // [2]
    const double* normals; const double* uniforms;
    double* host_state;                                                           // [parts * 12]: publish_result's pinned target, in and out
    int32_t* host_flags;                                                          // [3]
};
enum {
    RBS_TEST_STEP_PROPAGATE = 0,        // b, recentre
    RBS_TEST_STEP_WEIGHTS = 1,          // updated
    RBS_TEST_STEP_RESAMPLE_GATHER = 2,  // b
    RBS_TEST_STEP_GATHER = 3,
    RBS_TEST_STEP_FILTER_TAIL = 4,      // b, updated
    RBS_TEST_STEP_FILTER_STEP = 5,      // b, updated, last
    RBS_TEST_STEP_MEAN = 6,
    RBS_TEST_STEP_RECENTRE = 7,         // part_new, in place
    RBS_TEST_STEP_SWAP = 8,             // no launch: swap_gathered
    RBS_TEST_STEP_COUNT = 9
};
struct rbs_test_filter_step { int32_t code, b, updated, last, recentre; };

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

extern "C" int32_t rbs_test_filter(const rbs_test_filter_io* io, const rbs_test_filter_step* steps, int32_t n_steps)
{
    namespace pr = rbs::probe;
    constexpr int kMaxSteps = 16;
    if (!io || !steps || n_steps < 0 || n_steps > kMaxSteps) return RBS_ERR_INVALID_ARGUMENT;
    if (io->n < 1 || io->n > rbt::kRedBlocks * rbt::kChunk || io->parts < 1 || io->parts > rbs::kMaxBodies) return RBS_ERR_INVALID_ARGUMENT;
    if (!io->part_old || !io->part_new || !io->part_old2 || !io->part_new2 || !io->noise || !io->noise2 || !io->logw || !io->ll || !io->ll2 ||
        !io->ll_new || !io->cdf || !io->idx || !io->idx2 || !io->parents || !io->deflt || !io->mean || !io->poses || !io->flag ||
        !io->host_state || !io->host_flags)
        return RBS_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < n_steps; ++k)
        if (steps[k].code < 0 || steps[k].code >= RBS_TEST_STEP_COUNT || steps[k].b < 0 || steps[k].b >= io->parts) return RBS_ERR_INVALID_ARGUMENT;
    const size_t n = (size_t)io->n, parts = (size_t)io->parts, D = parts * rbt::kBody, P6 = parts * 6;
    pr::Buffers B;
    rbt::TrackerDev T{};
    T.n = io->n; T.parts = io->parts; T.D = (int)D;
    for (int k = 0; k < 6; ++k) T.sigma[k] = io->sigma[k];
    T.vf = io->vf; T.max_kl = io->max_kl; T.seed = io->seed; T.frame = io->frame;
    T.part_old = B.make<double>(n * D, io->part_old);    T.part_new = B.make<double>(n * D, io->part_new);
    T.part_old2 = B.make<double>(n * D, io->part_old2);  T.part_new2 = B.make<double>(n * D, io->part_new2);
    T.noise = B.make<double>(n * P6, io->noise);         T.noise2 = B.make<double>(n * P6, io->noise2);
    T.logw = B.make<double>(n, io->logw);                T.ll = B.make<double>(n, io->ll);
    T.ll2 = B.make<double>(n, io->ll2);                  T.ll_new = B.make<double>(n, io->ll_new);
    T.cdf = B.make<double>(n, io->cdf);
    T.idx = B.make<int>(n, io->idx);                     T.idx2 = B.make<int>(n, io->idx2);
    T.parents = B.make<int>(n, io->parents);
    T.deflt = B.make<double>(D, io->deflt);              T.mean = B.make<double>(D + parts * 9, io->mean);
    T.poses = B.make<double>(n * parts * 12, io->poses); T.flag = B.make<int>(2, io->flag);
    T.red = B.make<double>((size_t)rbt::kRedBlocks * (3 + D));
    if (io->normals) T.normals = B.make<double>(n * P6, io->normals);
    if (io->uniforms) T.uniforms = B.make<double>(n * parts, io->uniforms);
    // publish_result's target: pinned host memory of this call's own, as rbs_tracker_create maps the tracker's
    double* h_state = nullptr;
    int* h_flags = nullptr;
    if (B.err == hipSuccess) B.err = hipHostMalloc(&h_state, sizeof(double) * D, hipHostMallocDefault);
    if (B.err == hipSuccess) B.err = hipHostMalloc(&h_flags, sizeof(int) * 4, hipHostMallocDefault);
    if (B.err == hipSuccess) {
        std::memcpy(h_state, io->host_state, sizeof(double) * D);
        for (int k = 0; k < 3; ++k) h_flags[k] = io->host_flags[k];
        B.err = hipHostGetDevicePointer(reinterpret_cast<void**>(&T.host_state), h_state, 0);
    }
    if (B.err == hipSuccess) B.err = hipHostGetDevicePointer(reinterpret_cast<void**>(&T.host_flags), h_flags, 0);
    if (B.err == hipSuccess) B.err = hipMemset(T.red, 0, sizeof(double) * (size_t)rbt::kRedBlocks * (3 + D));
    if (B.err == hipSuccess) {
        hipStream_t s = nullptr;
        for (int k = 0; k < n_steps; ++k) {
            const rbs_test_filter_step& q = steps[k];
            switch (q.code) {
            case RBS_TEST_STEP_PROPAGATE: launch_propagate(T, q.b, q.recentre ? 1 : 0, s); break;
            case RBS_TEST_STEP_WEIGHTS: launch_weights(T, q.updated ? 1 : 0, s); break;
            case RBS_TEST_STEP_RESAMPLE_GATHER: launch_resample_gather(T, q.b, s); break;
            case RBS_TEST_STEP_GATHER: launch_gather(T, s); break;
            case RBS_TEST_STEP_FILTER_TAIL: launch_filter_tail(T, q.b, q.updated ? 1 : 0, s); break;
            case RBS_TEST_STEP_FILTER_STEP: launch_filter_step(T, q.b, q.updated ? 1 : 0, q.last ? 1 : 0, s); break;
            case RBS_TEST_STEP_MEAN: launch_mean(T, s); break;
            case RBS_TEST_STEP_RECENTRE: launch_recentre(T, T.part_new, s); break;
            default: swap_gathered(T); break;
            }
        }
        B.ran();
    }
    B.fetch(io->part_old, T.part_old, n * D);    B.fetch(io->part_new, T.part_new, n * D);
    B.fetch(io->part_old2, T.part_old2, n * D);  B.fetch(io->part_new2, T.part_new2, n * D);
    B.fetch(io->noise, T.noise, n * P6);         B.fetch(io->noise2, T.noise2, n * P6);
    B.fetch(io->logw, T.logw, n);                B.fetch(io->ll, T.ll, n);
    B.fetch(io->ll2, T.ll2, n);                  B.fetch(io->cdf, T.cdf, n);
    B.fetch(io->idx, T.idx, n);                  B.fetch(io->idx2, T.idx2, n);
    B.fetch(io->parents, T.parents, n);
    B.fetch(io->deflt, T.deflt, D);              B.fetch(io->mean, T.mean, D + parts * 9);
    B.fetch(io->poses, T.poses, n * parts * 12); B.fetch(io->flag, T.flag, 2);
    if (B.err == hipSuccess) {
        std::memcpy(io->host_state, h_state, sizeof(double) * D);
        for (int k = 0; k < 3; ++k) io->host_flags[k] = h_flags[k];
    }
    if (h_state) (void)hipHostFree(h_state);
    if (h_flags) (void)hipHostFree(h_flags);
    return B.status();
}
