// host_filter.h -- the chisel_hip_depth_filter_* entry points (included by chisel_hip.hip): DepthFilter, depth_filter.cpp.
// Kernels: kernels_filter.h.
extern "C" {

// ---- DepthFilter (depth_filter.cpp) ----------------------------------------------------------------------------------------
struct chisel_hip_depth_filter {
    int device = 0;
    int height = 0, width = 0;
    FilterView view{};                                       // a, b, mu, cov: copies of the four below
    DeviceBuffer<double> a, b, mu, cov;
    DeviceBuffer<double> stage_mu, stage_cov, stage_out;     // host arrays pass through these
};
int chisel_hip_depth_filter_create(int height, int width, int device_id, chisel_hip_depth_filter **out) {
    if (!out || height <= 0 || width <= 0 || (int64_t)height * width > (1 << 28)) return fail(CHISEL_HIP_ERR_INVALID, "bad filter size");
    if (const int rc = open_device(device_id, &device_id)) return rc;
    chisel_hip_depth_filter *f = new chisel_hip_depth_filter();
    f->device = device_id; f->height = height; f->width = width;
    const size_t n = (size_t)height * width;
    f->view.n = (int)n;
    f->view.inv_depth_range = 100 - 0.01;  // m_nMaxInvDepth - m_nMinInvDepth, depth_filter.cpp:138-141
    for (DeviceBuffer<double> *p : {&f->a, &f->b, &f->mu, &f->cov, &f->stage_mu, &f->stage_cov, &f->stage_out})
        if (p->alloc(n) != hipSuccess) {
            chisel_hip_depth_filter_destroy(f);
            return fail(CHISEL_HIP_ERR_HIP, "hipMalloc failed");
        }
    f->view.a = f->a.get(); f->view.b = f->b.get(); f->view.mu = f->mu.get(); f->view.cov = f->cov.get();
    hipLaunchKernelGGL(filter_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, f->view);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    *out = f;
    return CHISEL_HIP_OK;
}
int chisel_hip_depth_filter_destroy(chisel_hip_depth_filter *f) {
    if (!f) return CHISEL_HIP_OK;
    (void)hipSetDevice(f->device);
    (void)hipDeviceSynchronize();
    delete f;
    return CHISEL_HIP_OK;
}
int chisel_hip_depth_filter_update(chisel_hip_depth_filter *f, const double *mu, const double *cov, double cov_all, int reciprocal,
                                   int on_device) {
    if (!f || !mu) return fail(CHISEL_HIP_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(f->device));
    const size_t n = (size_t)f->view.n;
    const double *d_mu = mu, *d_cov = cov;
    if (!on_device) {
        HIP_TRY(hipMemcpyAsync(f->stage_mu.get(), mu, n * sizeof(double), hipMemcpyHostToDevice, 0));
        d_mu = f->stage_mu.get();
        if (cov) {
            HIP_TRY(hipMemcpyAsync(f->stage_cov.get(), cov, n * sizeof(double), hipMemcpyHostToDevice, 0));
            d_cov = f->stage_cov.get();
        }
    }
    hipLaunchKernelGGL(filter_update_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, f->view, d_mu, d_cov, cov_all, reciprocal);
    HIP_TRY(hipGetLastError());
    // host form: the staging copies have consumed mu and cov before this returns, so the caller may overwrite or free them (from
    // page-locked memory the copy is a DMA that is still reading its source when hipMemcpyAsync returns); the device form returns at once
    if (!on_device) HIP_TRY(hipStreamSynchronize(0));
    return CHISEL_HIP_OK;  // stream 0: ordered against the next call; reads wait
}
int chisel_hip_depth_filter_read(chisel_hip_depth_filter *f, int which, double *dst, int dst_on_device) {
    if (!f || !dst || which < 0 || which > 6) return fail(CHISEL_HIP_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(f->device));
    const size_t n = (size_t)f->view.n;
    double *d_out = dst_on_device ? dst : f->stage_out.get();
    hipLaunchKernelGGL(filter_read_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, f->view, which, d_out);
    HIP_TRY(hipGetLastError());
    if (!dst_on_device) HIP_TRY(hipMemcpyAsync(dst, d_out, n * sizeof(double), hipMemcpyDeviceToHost, 0));
    HIP_TRY(hipStreamSynchronize(0));
    return CHISEL_HIP_OK;
}
int chisel_hip_depth_filter_device(const chisel_hip_depth_filter *f, int *device) {
    if (!f || !device) return fail(CHISEL_HIP_ERR_INVALID, "null argument");
    *device = f->device;
    return CHISEL_HIP_OK;
}

}  // extern "C"
