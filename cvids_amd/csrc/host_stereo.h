// host_stereo.h -- the chisel_hip_stereo_* entry points (included by chisel_hip.hip): StereoMapper on prepared images and its
// raw-image path.  Kernels: kernels_stereo.h, kernels_stereo_prep.h.
namespace {
// a buffer of the raw-image path: one that is already there is kept (set_camera again), a new one is zeroed where its first reader expects that
template <class T>
int stereo_ensure(DeviceBuffer<T> &b, size_t n, bool zero) {
    if (b) return CHISEL_HIP_OK;
    HIP_TRY(b.alloc(n));
    if (zero) HIP_TRY(hipMemset(b.get(), 0, n * sizeof(T)));
    return CHISEL_HIP_OK;
}
}  // namespace

extern "C" {

// ---- StereoMapper (sgm_stereo_mapper.cpp, calc_cost.cu) ---------------------------------------------------------------------
struct chisel_hip_stereo {
    int device = 0;
    int width = 0, height = 0;
    int measurement_cnt = 0;  // m_nMeasurementCount: reset by InitReference only (sgm_stereo_mapper.cpp:121)
    bool has_reference = false;
    StereoParams prm{};
    StereoView view{};                               // its pointers: copies of ref, match, p2w, cost, sgm, depth below
    DeviceBuffer<float> ref, match, p2w;
    DeviceBuffer<float> cost, sgm, depth;            // the two volumes [H][W][STEREO_DEP_CNT] and WTA's result
    DeviceBuffer<float> stage_a, stage_b;            // host sparse maps pass through these
    DeviceBuffer<double> stage_out;                  // read-out 3 to the host
    // the raw-image path (chisel_hip_stereo_set_camera and after): allocated by the first set_camera
    bool has_camera = false;
    int real_w = 0, real_h = 0;
    double K1[4] = {}, K2[4] = {};                   // fx, fy, cx, cy scaled to the work size (InitIntrinsic)
    DeviceBuffer<short2> map_xy[2];                  // undistort maps of camera 1 (reference) and 2 (match), CV_16SC2 + CV_16UC1
    DeviceBuffer<uint16_t> map_f[2];
    DeviceBuffer<uint8_t> raw;                       // real_w x real_h input staged contiguous
    DeviceBuffer<uint8_t> small;                     // the W x H resize
    DeviceBuffer<int> sob_g, sob_x, sob_y;
    DeviceBuffer<long long> sob_partials;
    DeviceBuffer<StereoPrepStats> stats;
    DeviceBuffer<uint8_t> mask_x, mask_y;
    DeviceBuffer<float> sparse_depth, sparse_dist;
    DeviceBuffer<double> pts_depth, pts_xy;          // bound points (BindSparsePoints)
    DeviceBuffer<SparsePoint> pts;
    int n_points = 0, pts_cap = 0;
    DeviceBuffer<float> depth_real;                  // Output's result at the camera size
    DeviceBuffer<double> stage_real;                 // read-out 5 to the host
};

void chisel_hip_stereo_default_params(chisel_hip_stereo_params *p) {
    if (!p) return;
    // dense_mapping_parameters.cpp:3-11; DEP_SAMPLE = 1.0f / (BASE_LINE * FOCAL), dense_mapping_parameters.h:24,36-37
    const float focal = (float)((461.6 + 460.3) / 2);
    const float base_line = 0.11f;
    *p = {16.0f, 64.0f, 8.0f, 1.0f, 1.0f, 1.0f, 15.0f, 1.0f / (base_line * focal)};
}

int chisel_hip_stereo_create(int width, int height, const chisel_hip_stereo_params *p, int device_id, chisel_hip_stereo **out) {
    if (!out || width < 2 || height < 2 || width > 16384 || height > 16384 || (int64_t)width * height > (1 << 24))
        return fail(CHISEL_HIP_ERR_INVALID, "bad stereo size");
    chisel_hip_stereo_params prm;
    if (p) prm = *p;
    else chisel_hip_stereo_default_params(&prm);
    if (!(prm.dep_sample > 0.0f) || !(prm.sgm_q1 != 0.0f) || !(prm.sgm_q2 != 0.0f)) return fail(CHISEL_HIP_ERR_INVALID, "bad stereo parameters");
    if (const int rc = open_device(device_id, &device_id)) return rc;
    chisel_hip_stereo *s = new chisel_hip_stereo();
    s->device = device_id; s->width = width; s->height = height;
    s->prm = {prm.pi1, prm.pi2, prm.tau_so, prm.sgm_q1, prm.sgm_q2, prm.var_scale, prm.sparse_ratio, prm.dep_sample};
    const size_t n = (size_t)width * height, nv = n * STEREO_DEP_CNT;
    hipError_t e = s->stage_out.alloc(n);
    for (DeviceBuffer<float> *b : {&s->ref, &s->match, &s->p2w, &s->stage_a, &s->stage_b, &s->depth})
        if (e == hipSuccess) e = b->alloc(n);
    for (DeviceBuffer<float> *b : {&s->cost, &s->sgm})
        if (e == hipSuccess) e = b->alloc(nv);
    if (e != hipSuccess) {
        chisel_hip_stereo_destroy(s);
        return fail(CHISEL_HIP_ERR_HIP, "hipMalloc failed");
    }
    s->view.w = width; s->view.h = height;
    s->view.ref = s->ref.get(); s->view.match = s->match.get(); s->view.p2w = s->p2w.get();
    s->view.cost = s->cost.get(); s->view.sgm = s->sgm.get(); s->view.depth = s->depth.get();
    // every image and volume starts zeroed, as after ClearRawCost
    const std::pair<void *, size_t> zeroed[] = {{s->ref.get(), n * sizeof(float)},       {s->match.get(), n * sizeof(float)},
                                                {s->p2w.get(), n * sizeof(float)},       {s->view.cost, nv * sizeof(float)},
                                                {s->view.sgm, nv * sizeof(float)}, {s->view.depth, n * sizeof(float)}};
    for (const auto &z : zeroed)
        if (e == hipSuccess) e = hipMemsetAsync(z.first, 0, z.second, 0);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        chisel_hip_stereo_destroy(s);
        return fail(CHISEL_HIP_ERR_HIP, std::string("zeroing the stereo state: ") + hipGetErrorString(e));
    }
    *out = s;
    return CHISEL_HIP_OK;
}

int chisel_hip_stereo_destroy(chisel_hip_stereo *s) {
    if (!s) return CHISEL_HIP_OK;
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();
    delete s;
    return CHISEL_HIP_OK;
}

static int stereo_upload(float *dst, const float *src, size_t n, int on_device) {
    HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(float), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, 0));
    return CHISEL_HIP_OK;
}

int chisel_hip_stereo_set_reference(chisel_hip_stereo *s, const float *ref, const float *p2_weight, int on_device) {
    if (!s || !ref || !p2_weight) return fail(CHISEL_HIP_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(s->device));
    const size_t n = (size_t)s->width * s->height;
    int rc = stereo_upload(s->ref.get(), ref, n, on_device);
    if (rc == CHISEL_HIP_OK) rc = stereo_upload(s->p2w.get(), p2_weight, n, on_device);
    if (rc != CHISEL_HIP_OK) return rc;
    if (!on_device) HIP_TRY(hipStreamSynchronize(0));
    s->measurement_cnt = 0;
    s->has_reference = true;
    return CHISEL_HIP_OK;
}

// Update's cost pass (sgm_stereo_mapper.cpp:153, :184-195) on the match image already in s->match.get()
static int stereo_run_cost(chisel_hip_stereo *s, const float R[9], const float t[3]) {
    const size_t n = (size_t)s->width * s->height;
    StereoPose P;
    memcpy(P.r, R, sizeof(P.r));
    memcpy(P.t, t, sizeof(P.t));
    s->measurement_cnt++;
    hipLaunchKernelGGL(stereo_cost_kernel, dim3((unsigned)((n + 1) / 2)), dim3(256), 0, 0, s->view, P, s->measurement_cnt, s->prm.dep_sample);
    HIP_TRY(hipGetLastError());
    return CHISEL_HIP_OK;
}

int chisel_hip_stereo_update(chisel_hip_stereo *s, const float *match, const float R[9], const float t[3], int on_device) {
    if (!s || !match || !R || !t) return fail(CHISEL_HIP_ERR_INVALID, "null argument");
    if (!s->has_reference) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_stereo_update before chisel_hip_stereo_set_reference");
    HIP_TRY(hipSetDevice(s->device));
    const size_t n = (size_t)s->width * s->height;
    int rc = stereo_upload(s->match.get(), match, n, on_device);
    if (rc == CHISEL_HIP_OK) rc = stereo_run_cost(s, R, t);
    if (rc != CHISEL_HIP_OK) return rc;
    if (!on_device) HIP_TRY(hipStreamSynchronize(0));  // the host image may go once this returns
    return CHISEL_HIP_OK;  // stream 0: ordered against the next call; reads wait
}

// Output's device half (sgm_stereo_mapper.cpp:366-382): FuseSparseInfo when given device sparse maps, then SGM and WTA
static int stereo_run_output(chisel_hip_stereo *s, const float *dd, const float *ds) {
    const int W = s->width, H = s->height;
    const size_t n = (size_t)W * H, nv = n * STEREO_DEP_CNT;
    if (dd) {
        hipLaunchKernelGGL(stereo_fuse_sparse_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, 0, s->view, dd, ds,
                           s->prm.sparse_ratio, s->prm.dep_sample);
        HIP_TRY(hipGetLastError());
    }
    // sgm2 (calc_cost.cu:507-546): right, left, down, up, in that order, each adding its path costs to the volume; the first
    // writes, which equals adding to the zeroed volume of sgm_stereo_mapper.cpp:371
    const SgmScan passes[4] = {
        {H, W, W, 1, 0},
        {H, W, W, -1, W - 1},
        {W, H, 1, W, 0},
        {W, H, 1, -W, (H - 1) * W},
    };
    for (int k = 0; k < 4; ++k) {
        const dim3 grid((unsigned)((passes[k].n_lines + 3) / 4));
        if (k == 0) hipLaunchKernelGGL(stereo_sgm_kernel<true>, grid, dim3(256), 0, 0, s->view, passes[k], s->prm);
        else hipLaunchKernelGGL(stereo_sgm_kernel<false>, grid, dim3(256), 0, 0, s->view, passes[k], s->prm);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(stereo_wta_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, 0, s->view, s->prm.var_scale, s->prm.dep_sample);
    HIP_TRY(hipGetLastError());
    return CHISEL_HIP_OK;
}

int chisel_hip_stereo_output(chisel_hip_stereo *s, const float *sparse_depth, const float *sparse_dist, int on_device) {
    if (!s || (!sparse_depth) != (!sparse_dist)) return fail(CHISEL_HIP_ERR_INVALID, "bad argument (sparse depth and distance go together)");
    HIP_TRY(hipSetDevice(s->device));
    const size_t n = (size_t)s->width * s->height;
    // FuseSparseInfo (sgm_stereo_mapper.cpp:366-368); without a prior every nDepth is -1 and it changes nothing
    const float *dd = sparse_depth, *ds = sparse_dist;
    if (sparse_depth && !on_device) {
        HIP_TRY(hipMemcpyAsync(s->stage_a.get(), sparse_depth, n * sizeof(float), hipMemcpyHostToDevice, 0));
        HIP_TRY(hipMemcpyAsync(s->stage_b.get(), sparse_dist, n * sizeof(float), hipMemcpyHostToDevice, 0));
        dd = s->stage_a.get();
        ds = s->stage_b.get();
    }
    const int rc = stereo_run_output(s, dd, ds);
    if (rc != CHISEL_HIP_OK) return rc;
    if (sparse_depth && !on_device) HIP_TRY(hipStreamSynchronize(0));
    return CHISEL_HIP_OK;
}

int chisel_hip_stereo_clear(chisel_hip_stereo *s) {
    if (!s) return fail(CHISEL_HIP_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(s->device));
    const size_t n = (size_t)s->width * s->height, nv = n * STEREO_DEP_CNT;
    HIP_TRY(hipMemsetAsync(s->view.cost, 0, nv * sizeof(float), 0));
    HIP_TRY(hipMemsetAsync(s->view.sgm, 0, nv * sizeof(float), 0));
    HIP_TRY(hipMemsetAsync(s->view.depth, 0, n * sizeof(float), 0));
    return CHISEL_HIP_OK;  // the measurement count stays (sgm_stereo_mapper.cpp:202-216)
}

int chisel_hip_stereo_read(chisel_hip_stereo *s, int which, void *dst, int dst_on_device) {
    if (!s || !dst || which < 0 || which > 5) return fail(CHISEL_HIP_ERR_INVALID, "bad argument");
    if (which >= 4 && !s->has_camera) return fail(CHISEL_HIP_ERR_INVALID, "read-outs 4 and 5 are at the camera size: chisel_hip_stereo_set_camera first");
    HIP_TRY(hipSetDevice(s->device));
    const size_t n = (size_t)s->width * s->height, n_real = (size_t)s->real_w * s->real_h;
    const hipMemcpyKind kind = dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (which == 0) HIP_TRY(hipMemcpyAsync(dst, s->view.cost, n * STEREO_DEP_CNT * sizeof(float), kind, 0));
    else if (which == 1) HIP_TRY(hipMemcpyAsync(dst, s->view.sgm, n * STEREO_DEP_CNT * sizeof(float), kind, 0));
    else if (which == 2) HIP_TRY(hipMemcpyAsync(dst, s->view.depth, n * sizeof(float), kind, 0));
    else if (which == 4) HIP_TRY(hipMemcpyAsync(dst, s->depth_real.get(), n_real * sizeof(float), kind, 0));
    else {
        const float *src = which == 3 ? s->view.depth : s->depth_real.get();
        const size_t m = which == 3 ? n : n_real;
        double *d_out = dst_on_device ? static_cast<double *>(dst) : (which == 3 ? s->stage_out.get() : s->stage_real.get());
        hipLaunchKernelGGL(stereo_widen_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, 0, src, d_out, (int)m);
        HIP_TRY(hipGetLastError());
        if (!dst_on_device) HIP_TRY(hipMemcpyAsync(dst, d_out, m * sizeof(double), hipMemcpyDeviceToHost, 0));
    }
    HIP_TRY(hipStreamSynchronize(0));
    return CHISEL_HIP_OK;
}

// ---- the raw-image path: InitIntrinsic, InitReference, Update, BindSparsePoints, Output with their OpenCV work on the device ------
// cv::invert(DECOMP_LU) of a 3 x 3 CV_64F matrix takes a closed form (core/src/lapack.cpp, cv::invert, n == 3): det3 expanded
// along the first row, d = 1. / det, then every entry of the adjugate (2 x 2 cofactor differences) times d.  false: det == 0.
static bool stereo_invert3(const double *m, double *o) {
#define M_(i, j) m[(i) * 3 + (j)]
    double d = M_(0, 0) * (M_(1, 1) * M_(2, 2) - M_(1, 2) * M_(2, 1)) - M_(0, 1) * (M_(1, 0) * M_(2, 2) - M_(1, 2) * M_(2, 0)) +
               M_(0, 2) * (M_(1, 0) * M_(2, 1) - M_(1, 1) * M_(2, 0));
    if (d == 0.) return false;
    d = 1. / d;
    o[0] = (M_(1, 1) * M_(2, 2) - M_(1, 2) * M_(2, 1)) * d;
    o[1] = (M_(0, 2) * M_(2, 1) - M_(0, 1) * M_(2, 2)) * d;
    o[2] = (M_(0, 1) * M_(1, 2) - M_(0, 2) * M_(1, 1)) * d;
    o[3] = (M_(1, 2) * M_(2, 0) - M_(1, 0) * M_(2, 2)) * d;
    o[4] = (M_(0, 0) * M_(2, 2) - M_(0, 2) * M_(2, 0)) * d;
    o[5] = (M_(0, 2) * M_(1, 0) - M_(0, 0) * M_(1, 2)) * d;
    o[6] = (M_(1, 0) * M_(2, 1) - M_(1, 1) * M_(2, 0)) * d;
    o[7] = (M_(0, 1) * M_(2, 0) - M_(0, 0) * M_(2, 1)) * d;
    o[8] = (M_(0, 0) * M_(1, 1) - M_(0, 1) * M_(1, 0)) * d;
#undef M_
    return true;
}

// 3 x 3 times 3 x cols (cols 3 or 1), every entry a0 b0 + a1 b1 + a2 b2 left to right; bt: b is 3 x 3 and used transposed
static void stereo_mul3(const double *a, const double *b, int cols, bool bt, double *o) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < cols; ++j) {
            const double b0 = bt ? b[j * 3 + 0] : b[0 * cols + j], b1 = bt ? b[j * 3 + 1] : b[1 * cols + j], b2 = bt ? b[j * 3 + 2] : b[2 * cols + j];
            o[i * cols + j] = a[i * 3 + 0] * b0 + a[i * 3 + 1] * b1 + a[i * 3 + 2] * b2;
        }
}

int chisel_hip_stereo_homography(const double K1[4], const double K2[4], const double Rr[9], const double tr[3], const double Rm[9],
                                 const double tm[3], float R[9], float t[3]) {
    if (!K1 || !K2 || !Rr || !tr || !Rm || !tm || !R || !t) return fail(CHISEL_HIP_ERR_INVALID, "null argument");
    const double k1[9] = {K1[0], 0.0, K1[2], 0.0, K1[1], K1[3], 0.0, 0.0, 1.0};
    const double k2[9] = {K2[0], 0.0, K2[2], 0.0, K2[1], K2[3], 0.0, 0.0, 1.0};
    double k1i[9], a[9], b[9], r[9], tt[3];
    if (!stereo_invert3(k1, k1i)) return fail(CHISEL_HIP_ERR_INVALID, "K1 is singular");
    stereo_mul3(k2, Rm, 3, true, a);  // K2 * Rm.t()
    stereo_mul3(a, Rr, 3, false, b);  // * Rr
    stereo_mul3(b, k1i, 3, false, r); // * K1.inv()
    const double d[3] = {tr[0] - tm[0], tr[1] - tm[1], tr[2] - tm[2]};
    stereo_mul3(a, d, 1, false, tt);  // K2 * Rm.t() * (tr - tm)
    for (int k = 0; k < 9; ++k) R[k] = (float)r[k];
    for (int k = 0; k < 3; ++k) t[k] = (float)tt[k];
    return CHISEL_HIP_OK;
}

// cvRound as x86-64 computes it (cvtsd2si): round half to even; NaN and values outside int give INT_MIN
static int stereo_cv_round(double v) {
    return (v >= -2147483648.5 && v < 2147483647.5) ? (int)std::nearbyint(v) : INT32_MIN;
}

// cv::undistort(src, dst, K, D, K) of OpenCV 4 (imgproc/src/undistort.dispatch.cpp), its map restated from the scalar loop of
// initUndistortRectifyMap with R = I and map type CV_16SC2: the rows go in stripes of min(max(1, 4096 / cols), rows); in each,
// Ar(1,2) = v0 - y and ir = Ar^-1 (stereo_invert3; Ar * I is Ar bit for bit); per row i of the stripe _x, _y, _w start at
// i * ir[1] + ir[2], i * ir[4] + ir[5], i * ir[7] + ir[8] and get += ir[0], ir[3], ir[6] column by column; w = 1. / _w,
// x = _x * w, y = _y * w; kr = (1 + ((k3 r2 + k2) r2 + k1) r2) / (1 + ((k6 r2 + k5) r2 + k4) r2) with k4..k6 = 0;
// xd = x kr + p1 2xy + p2 (r2 + 2 x2), yd = y kr + p1 (r2 + 2 y2) + p2 2xy (the thin-prism terms s1..s4 are 0 and the tilt is the
// identity: they change at most the sign of a zero, which u = fx xd + u0 removes); u, v with fx, fy, u0, v0 of the unmodified
// A; iu = cvRound(u * 32), iv = cvRound(v * 32); map (short)(iu >> 5), (short)(iv >> 5) and (iv & 31) * 32 + (iu & 31).
static void stereo_undistort_map(int W, int H, const double K[4], const double D[5], short2 *xy, uint16_t *f) {
    const double fx = K[0], fy = K[1], u0 = K[2], v0 = K[3];
    const double k1 = D[0], k2 = D[1], p1 = D[2], p2 = D[3], k3 = D[4], k4 = 0.0, k5 = 0.0, k6 = 0.0;
    const int stripe0 = std::min(std::max(1, 4096 / std::max(W, 1)), H);
    for (int y = 0; y < H; y += stripe0) {
        const int rows = std::min(stripe0, H - y);
        const double Ar[9] = {fx, 0.0, u0, 0.0, fy, v0 - y, 0.0, 0.0, 1.0};
        double ir[9];
        if (!stereo_invert3(Ar, ir)) std::fill(ir, ir + 9, 0.0);  // cv::invert leaves a singular matrix's inverse zeroed
        for (int i = 0; i < rows; ++i) {
            double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
            for (int j = 0; j < W; ++j, _x += ir[0], _y += ir[3], _w += ir[6]) {
                const double w = 1. / _w, x = _x * w, yy = _y * w;
                const double x2 = x * x, y2 = yy * yy;
                const double r2 = x2 + y2, _2xy = 2 * x * yy;
                const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
                const double xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2);
                const double yd = yy * kr + p1 * (r2 + 2 * y2) + p2 * _2xy;
                const double u = fx * xd + u0, v = fy * yd + v0;
                const int iu = stereo_cv_round(u * 32), iv = stereo_cv_round(v * 32);
                const size_t k = (size_t)(y + i) * W + j;
                xy[k] = make_short2((short)(iu >> 5), (short)(iv >> 5));
                f[k] = (uint16_t)((iv & 31) * 32 + (iu & 31));
            }
        }
    }
}

int chisel_hip_stereo_set_camera(chisel_hip_stereo *s, int real_w, int real_h, const double K1[4], const double D1[5], const double K2[4],
                                 const double D2[5]) {
    if (!s || !K1 || !D1 || !K2 || !D2) return fail(CHISEL_HIP_ERR_INVALID, "null argument");
    if (real_w < 2 || real_h < 2 || real_w > 16384 || real_h > 16384 || (int64_t)real_w * real_h > (1 << 26))
        return fail(CHISEL_HIP_ERR_INVALID, "bad camera image size");
    const int W = s->width, H = s->height;
    if (W < 9 || H < 9) return fail(CHISEL_HIP_ERR_INVALID, "the raw-image path needs a work size of at least 9 x 9 (the border of the 9-tap Sobel)");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());  // buffers below may be in use by queued work
    const size_t n = (size_t)W * H, n_real = (size_t)real_w * real_h;
    const size_t n_blocks = (size_t)((W + SOBEL_TILE - 1) / SOBEL_TILE) * ((H + SOBEL_TILE - 1) / SOBEL_TILE);
    if (s->real_w != real_w || s->real_h != real_h) {
        s->raw.reset();
        s->depth_real.reset();
        s->stage_real.reset();
    }
    // already allocated: keep.  On a failure what was allocated stays with s (its destructor frees it) and the camera is not set.
    int rc = CHISEL_HIP_OK;
    for (int c = 0; c < 2; ++c) {
        if ((rc = stereo_ensure(s->map_xy[c], n, false))) return rc;
        if ((rc = stereo_ensure(s->map_f[c], n, false))) return rc;
    }
    if ((rc = stereo_ensure(s->small, n, false))) return rc;
    for (DeviceBuffer<int> *b : {&s->sob_g, &s->sob_x, &s->sob_y})
        if ((rc = stereo_ensure(*b, n, false))) return rc;
    if ((rc = stereo_ensure(s->sob_partials, n_blocks * SOBEL_N_STATS, false))) return rc;
    if ((rc = stereo_ensure(s->stats, 1, true))) return rc;
    for (DeviceBuffer<uint8_t> *b : {&s->mask_x, &s->mask_y})
        if ((rc = stereo_ensure(*b, n, true))) return rc;
    for (DeviceBuffer<float> *b : {&s->sparse_depth, &s->sparse_dist})
        if ((rc = stereo_ensure(*b, n, false))) return rc;
    if ((rc = stereo_ensure(s->raw, n_real, false))) return rc;
    if ((rc = stereo_ensure(s->depth_real, n_real, true))) return rc;
    if ((rc = stereo_ensure(s->stage_real, n_real, false))) return rc;
    // InitIntrinsic (sgm_stereo_mapper.cpp:31-45): fx, cx / (real_w / W), fy, cy / (real_h / H)
    const double sx = (double)real_w / (double)W, sy = (double)real_h / (double)H;
    const double k1[4] = {K1[0] / sx, K1[1] / sy, K1[2] / sx, K1[3] / sy}, k2[4] = {K2[0] / sx, K2[1] / sy, K2[2] / sx, K2[3] / sy};
    std::vector<short2> xy(n);
    std::vector<uint16_t> f(n);
    for (int c = 0; c < 2; ++c) {
        stereo_undistort_map(W, H, c == 0 ? k1 : k2, c == 0 ? D1 : D2, xy.data(), f.data());
        HIP_TRY(hipMemcpy(s->map_xy[c].get(), xy.data(), n * sizeof(short2), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(s->map_f[c].get(), f.data(), n * sizeof(uint16_t), hipMemcpyHostToDevice));
    }
    memcpy(s->K1, k1, sizeof(k1));
    memcpy(s->K2, k2, sizeof(k2));
    s->real_w = real_w;
    s->real_h = real_h;
    s->has_camera = true;
    return CHISEL_HIP_OK;
}

// cv::resize of the real_w x real_h mono8 image to W x H (condition_color_kernel), then cv::undistort with camera `cam` and
// convertTo(CV_32F) into dst
static int stereo_prepare(chisel_hip_stereo *s, const uint8_t *img, int step, int on_device, int cam, float *dst) {
    const int W = s->width, H = s->height, w0 = s->real_w, h0 = s->real_h;
    const uint8_t *src = img;
    if (!on_device || step != w0) {
        HIP_TRY(hipMemcpy2DAsync(s->raw.get(), w0, img, step, w0, h0, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, 0));
        src = s->raw.get();
    }
    hipLaunchKernelGGL(condition_color_kernel, dim3((W + 255) / 256, H), dim3(256), 0, 0, src, w0, h0, 1, s->small.get(), W, H);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(stereo_remap_kernel, dim3((unsigned)(((size_t)W * H + 255) / 256)), dim3(256), 0, 0, s->small.get(), W, H, s->map_xy[cam].get(),
                       s->map_f[cam].get(), dst);
    HIP_TRY(hipGetLastError());
    return CHISEL_HIP_OK;
}

static int stereo_check_image(chisel_hip_stereo *s, const uint8_t *img, int step, const char *what) {
    if (!s || !img) return fail(CHISEL_HIP_ERR_INVALID, "null argument");
    if (!s->has_camera) return fail(CHISEL_HIP_ERR_INVALID, std::string(what) + " before chisel_hip_stereo_set_camera");
    if (step < s->real_w) return fail(CHISEL_HIP_ERR_INVALID, "row step shorter than the camera image");
    return CHISEL_HIP_OK;
}

int chisel_hip_stereo_set_reference_image(chisel_hip_stereo *s, const uint8_t *img, int step, int on_device) {
    int rc = stereo_check_image(s, img, step, "chisel_hip_stereo_set_reference_image");
    if (rc != CHISEL_HIP_OK) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const int W = s->width, H = s->height, n = W * H;
    rc = stereo_prepare(s, img, step, on_device, 0, s->ref.get());
    if (rc != CHISEL_HIP_OK) return rc;
    const dim3 tiles((W + SOBEL_TILE - 1) / SOBEL_TILE, (H + SOBEL_TILE - 1) / SOBEL_TILE);
    hipLaunchKernelGGL(stereo_sobel_kernel, tiles, dim3(256), 0, 0, s->ref.get(), W, H, s->sob_g.get(), s->sob_x.get(), s->sob_y.get(), s->sob_partials.get());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(stereo_prep_stats_kernel, dim3(1), dim3(256), 0, 0, s->sob_partials.get(), (int)(tiles.x * tiles.y), n, s->stats.get());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(stereo_prep_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, s->sob_g.get(), s->sob_x.get(), s->sob_y.get(), s->stats.get(), n, s->p2w.get(),
                       s->mask_x.get(), s->mask_y.get());
    HIP_TRY(hipGetLastError());
    if (!on_device) HIP_TRY(hipStreamSynchronize(0));
    s->measurement_cnt = 0;  // sgm_stereo_mapper.cpp:121
    s->has_reference = true;
    return CHISEL_HIP_OK;
}

int chisel_hip_stereo_update_image(chisel_hip_stereo *s, const uint8_t *img, int step, const double ref_R_wc[9], const double ref_t_wc[3],
                                   const double match_R_wc[9], const double match_t_wc[3], int on_device) {
    int rc = stereo_check_image(s, img, step, "chisel_hip_stereo_update_image");
    if (rc != CHISEL_HIP_OK) return rc;
    if (!ref_R_wc || !ref_t_wc || !match_R_wc || !match_t_wc) return fail(CHISEL_HIP_ERR_INVALID, "null pose");
    if (!s->has_reference) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_stereo_update_image before a reference image");
    float R[9], t[3];
    rc = chisel_hip_stereo_homography(s->K1, s->K2, ref_R_wc, ref_t_wc, match_R_wc, match_t_wc, R, t);  // :179-182
    if (rc != CHISEL_HIP_OK) return rc;
    HIP_TRY(hipSetDevice(s->device));
    rc = stereo_prepare(s, img, step, on_device, 1, s->match.get());
    if (rc == CHISEL_HIP_OK) rc = stereo_run_cost(s, R, t);
    if (rc != CHISEL_HIP_OK) return rc;
    if (!on_device) HIP_TRY(hipStreamSynchronize(0));
    return CHISEL_HIP_OK;
}

int chisel_hip_stereo_bind_sparse_points(chisel_hip_stereo *s, const double *depth, const double *xy, int n) {
    if (!s || n < 0 || n > (1 << 24) || (n > 0 && (!depth || !xy))) return fail(CHISEL_HIP_ERR_INVALID, "bad argument");
    if (!s->has_camera) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_stereo_bind_sparse_points before chisel_hip_stereo_set_camera");
    HIP_TRY(hipSetDevice(s->device));
    if (n > s->pts_cap) {
        HIP_TRY(hipDeviceSynchronize());  // a queued Output may still read the old points
        s->pts_depth.reset();
        s->pts_xy.reset();
        s->pts.reset();
        s->pts_cap = 0;
        const int cap = std::max(n, 1024);
        int rc = stereo_ensure(s->pts_depth, (size_t)cap, false);
        if (rc == CHISEL_HIP_OK) rc = stereo_ensure(s->pts_xy, (size_t)cap * 2, false);
        if (rc == CHISEL_HIP_OK) rc = stereo_ensure(s->pts, (size_t)cap, false);
        if (rc != CHISEL_HIP_OK) {
            s->n_points = 0;
            return rc;
        }
        s->pts_cap = cap;
    }
    if (n > 0) {  // hipMemcpy from pageable memory: ordered after queued work, done when it returns (BindSparsePoints copies)
        HIP_TRY(hipMemcpy(s->pts_depth.get(), depth, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(s->pts_xy.get(), xy, (size_t)n * 2 * sizeof(double), hipMemcpyHostToDevice));
    }
    s->n_points = n;
    return CHISEL_HIP_OK;
}

static SparseRatios stereo_sparse_ratios() {
    SparseRatios R;
    for (int u = -SPARSE_WIN; u <= SPARSE_WIN; ++u)
        for (int v = -SPARSE_WIN; v <= SPARSE_WIN; ++v) {
            double r = (1.0 - (std::sqrt((double)(u * u + v * v)) / (SPARSE_WIN * 1.414)));  // sgm_stereo_mapper.cpp:346-347
            r = r * r;
            const int b = (u + SPARSE_WIN) * SPARSE_SIDE + (v + SPARSE_WIN);
            R.ratio[b] = r;
            R.stored[b] = (float)(r * r);  // :350
        }
    return R;
}

int chisel_hip_stereo_output_image(chisel_hip_stereo *s) {
    if (!s) return fail(CHISEL_HIP_ERR_INVALID, "null argument");
    if (!s->has_camera) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_stereo_output_image before chisel_hip_stereo_set_camera");
    HIP_TRY(hipSetDevice(s->device));
    const int W = s->width, H = s->height, n = s->n_points;
    static const SparseRatios ratios = stereo_sparse_ratios();
    // 1. the sparse prior (:229-357): -1 / 0 where no point writes
    if (n > 0) {
        hipLaunchKernelGGL(stereo_sparse_points_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, s->pts_depth.get(), s->pts_xy.get(), n, W, H,
                           (double)s->real_h / (double)H, (double)s->real_w / (double)W, s->mask_x.get(), s->mask_y.get(), s->pts.get());
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(stereo_sparse_raster_kernel, dim3((W + 15) / 16, (H + 15) / 16), dim3(256), 0, 0, s->pts.get(), n, W, H, ratios,
                       s->sparse_depth.get(), s->sparse_dist.get());
    HIP_TRY(hipGetLastError());
    // 2-4. FuseSparseInfo (all -1 without points: it changes nothing and is skipped), SGM, WTA
    const int rc = stereo_run_output(s, n > 0 ? s->sparse_depth.get() : nullptr, s->sparse_dist.get());
    if (rc != CHISEL_HIP_OK) return rc;
    // 5. cv::resize to the camera size (:409)
    hipLaunchKernelGGL(stereo_resize_f32_kernel, dim3((s->real_w + 255) / 256, s->real_h), dim3(256), 0, 0, s->view.depth, W, H, s->depth_real.get(),
                       s->real_w, s->real_h);
    HIP_TRY(hipGetLastError());
    return CHISEL_HIP_OK;
}

int chisel_hip_debug_stereo_prep(chisel_hip_stereo *s, int which, void *dst) {
    if (!s || !dst || which < 0 || which > 6) return fail(CHISEL_HIP_ERR_INVALID, "bad argument");
    if (which >= 3 && !s->has_camera) return fail(CHISEL_HIP_ERR_INVALID, "no camera set");
    HIP_TRY(hipSetDevice(s->device));
    const size_t n = (size_t)s->width * s->height;
    const void *src[7] = {s->ref.get(), s->match.get(), s->p2w.get(), s->mask_x.get(), s->mask_y.get(), s->sparse_depth.get(), s->sparse_dist.get()};
    HIP_TRY(hipMemcpy(dst, src[which], n * (which == 3 || which == 4 ? 1 : sizeof(float)), hipMemcpyDeviceToHost));
    return CHISEL_HIP_OK;
}

}  // extern "C"
