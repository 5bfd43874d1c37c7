// host_align.h -- chisel_hip_align_terms, chisel_hip_align_solve and chisel_hip_align_depth (included by chisel_hip.hip; the kernels:
// kernels_align.h; DESIGN.md "Aligning a frame to the map" is the definition).  The map is only read.  The terms are evaluated by one
// launch chain on the map's stream -- align_terms_kernel, then one align_reduce_kernel per further level of the summation tree -- into
// buffers the map owns; the solver and the pose update are host code in double, written in the order the definition states.
#pragma once

namespace {
namespace align {

// A xi = -b with A = the symmetric matrix of terms[0..20] + damping terms[28] I and b = terms[21..26], by Cholesky A = L L^T;
// false: a pivot s with !(s > 1e-12 max_j A_jj)
bool solve(const double terms[32], double damping, double xi[6]) {
    double A[6][6], L[6][6] = {};
    int t = 0;
    for (int a = 0; a < 6; a++)
        for (int b = a; b < 6; b++) A[a][b] = A[b][a] = terms[t++];
    const double add = damping * terms[28];
    double largest = 0.0;
    for (int j = 0; j < 6; j++) {
        A[j][j] += add;
        if (j == 0 || A[j][j] > largest) largest = A[j][j];
    }
    const double floor_s = 1e-12 * largest;
    for (int j = 0; j < 6; j++) {
        double s = A[j][j];
        for (int k = 0; k < j; k++) s -= L[j][k] * L[j][k];
        if (!(s > floor_s)) return false;
        L[j][j] = sqrt(s);
        for (int i = j + 1; i < 6; i++) {
            double v = A[i][j];
            for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
    double y[6];
    for (int i = 0; i < 6; i++) {
        double v = -terms[21 + i];
        for (int k = 0; k < i; k++) v -= L[i][k] * y[k];
        y[i] = v / L[i][i];
    }
    for (int i = 5; i >= 0; i--) {
        double v = y[i];
        for (int k = i + 1; k < 6; k++) v -= L[k][i] * xi[k];
        xi[i] = v / L[i][i];
    }
    return true;
}

double norm3(const double *a) { return sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]); }

// pose (row-major 3 x 4) <- exp(xi) pose, the left perturbation p' = p + v + w x p: R <- R_d R, t <- R_d t + v with Rodrigues' R_d
void apply(const double xi[6], double pose[12]) {
    const double *v = xi, *w = xi + 3;
    const double theta = norm3(w);
    const double K[3][3] = {{0.0, -w[2], w[1]}, {w[2], 0.0, -w[0]}, {-w[1], w[0], 0.0}};
    double Rd[3][3];
    const bool tiny = theta <= 1e-12;
    const double a = tiny ? 1.0 : sin(theta) / theta, b = tiny ? 0.0 : (1.0 - cos(theta)) / (theta * theta);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double k2 = (K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j];
            Rd[i][j] = ((i == j ? 1.0 : 0.0) + a * K[i][j]) + b * k2;
        }
    double out[12];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 4; j++) out[4 * i + j] = (Rd[i][0] * pose[j] + Rd[i][1] * pose[4 + j]) + Rd[i][2] * pose[8 + j];
        out[4 * i + 3] += v[i];
    }
    memcpy(pose, out, sizeof(out));
}

// what the entries refuse, in chisel_hip_query_points' order; 0 = go on
int refusal(chisel_hip_map *m, const chisel_hip_depth_frame *f, const char *name) {
    const int rc = query_refusal(m, name, "reads the voxels around every pixel's point");
    if (rc) return rc;
    if (!f || !f->depth) return fail(CHISEL_HIP_ERR_INVALID, std::string(name) + ": null frame or depth image");
    if (const char *why = frame_image_refusal(f->depth, f->width, f->height)) return fail(CHISEL_HIP_ERR_INVALID, std::string(name) + ": " + why);
    return CHISEL_HIP_OK;
}

// the launch chain: 32 doubles at d_terms (device), on the map's stream, nothing waited for
int launch_terms(chisel_hip_map *m, const chisel_hip_depth_frame *f, const float pose[12], const float *d_depth, float max_residual, double *d_terms) {
    const int n = f->width * f->height;
    auto &A = m->align_mem;
    size_t need = 0;
    for (int g = (n + 255) / 256; g > 1; g = (g + 255) / 256) need += (size_t)ALIGN_SUMS * g;
    if (const int rc = grow_buffer(A.partials, need, m->stream)) return rc;
    AlignCamera cam;
    cam.cam = pixel_camera(pose, f->fx, f->fy, f->cx, f->cy);
    cam.near_plane = f->near_plane; cam.far_plane = f->far_plane;
    cam.max_residual = max_residual;
    cam.width = f->width;
    HIP_TRY(hipMemsetAsync(d_terms, 0, ALIGN_TERMS * sizeof(double), m->stream));  // ([30] and [31]; the sums are stored over the rest)
    const MeshParams P = mesh_params(m);
    int groups = (n + 255) / 256;
    double *level = groups > 1 ? A.partials.get() : d_terms;
    FOR_CHUNK_SIZE(m->N, hipLaunchKernelGGL(align_terms_kernel<N>, dim3((unsigned)groups), dim3(256), 0, m->stream, m->view, P, cam, d_depth, n, level, groups));
    HIP_TRY(hipGetLastError());
    while (groups > 1) {
        const int next = (groups + 255) / 256;
        double *out = next > 1 ? level + (size_t)ALIGN_SUMS * groups : d_terms;
        hipLaunchKernelGGL(align_reduce_kernel, dim3((unsigned)next, ALIGN_SUMS), dim3(256), 0, m->stream, level, groups, out);
        HIP_TRY(hipGetLastError());
        level = out;
        groups = next;
    }
    return CHISEL_HIP_OK;
}

int ensure_terms(chisel_hip_map *m) {
    if (!m->align_mem.terms) HIP_TRY(m->align_mem.terms.alloc(ALIGN_TERMS));
    return CHISEL_HIP_OK;
}

}  // namespace align
}  // namespace

extern "C" {

int chisel_hip_align_terms(chisel_hip_map *m, const chisel_hip_depth_frame *frame, float max_residual, double *terms, int terms_on_device) {
    SETTLE(m);
    {
        int rc_r = align::refusal(m, frame, "chisel_hip_align_terms");
        if (rc_r) return rc_r;
    }
    if (!terms) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_align_terms: null terms");
    HIP_TRY(hipSetDevice(m->device));
    {
        int rc_m = check_mesh_totals(m);  // a recompute in flight reads the voxels as they are
        if (rc_m) return rc_m;
    }
    const float *d_depth = nullptr;
    {
        int rc_s = stage_depth(m, frame, &d_depth);
        if (rc_s) return rc_s;
        if (!terms_on_device && (rc_s = align::ensure_terms(m))) return rc_s;
        if ((rc_s = wait_for_input(m, m->stream))) return rc_s;  // chisel_hip_wait_event / _order_map_after_stream: the image is ready behind it
    }
    double *d_terms = terms_on_device ? terms : m->align_mem.terms.get();
    int rc = align::launch_terms(m, frame, frame->pose, d_depth, max_residual, d_terms);
    if (rc == CHISEL_HIP_OK && !terms_on_device) {
        hipError_t e = hipMemcpyAsync(terms, d_terms, ALIGN_TERMS * sizeof(double), hipMemcpyDeviceToHost, m->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
        if (e != hipSuccess) rc = fail(CHISEL_HIP_ERR_HIP, std::string("chisel_hip_align_terms: ") + hipGetErrorString(e));
    } else if (rc != CHISEL_HIP_OK && !frame->on_device) {
        (void)hipStreamSynchronize(m->stream);  // (the caller's image may be freed on return)
    }
    if (rc == CHISEL_HIP_OK && terms_on_device && !frame->on_device) HIP_TRY(hipStreamSynchronize(m->stream));  // the copy of the host image is over on return
    return rc;
}

int chisel_hip_align_solve(const double terms[32], double damping, double xi[6]) {
    if (!terms || !xi) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_align_solve: null argument");
    double x[6] = {};
    if (!align::solve(terms, damping, x)) return fail(CHISEL_HIP_ERR_UNSUPPORTED, "chisel_hip_align_solve: the normal equations are degenerate (a Cholesky pivot at or below 1e-12 of the largest diagonal entry)");
    memcpy(xi, x, sizeof(x));
    return CHISEL_HIP_OK;
}

int chisel_hip_align_depth(chisel_hip_map *m, const chisel_hip_depth_frame *frame, const chisel_hip_align_params *params, chisel_hip_align_result *result) {
    static_assert(sizeof(chisel_hip_align_params) == 40 && sizeof(chisel_hip_align_result) == 664, "chisel_hip_align_params / _result layout");
    SETTLE(m);
    {
        int rc_r = align::refusal(m, frame, "chisel_hip_align_depth");
        if (rc_r) return rc_r;
    }
    if (!params || !result) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_align_depth: null params or result");
    if (params->max_iterations < 1) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_align_depth: max_iterations < 1");
    HIP_TRY(hipSetDevice(m->device));
    {
        int rc_m = check_mesh_totals(m);
        if (rc_m) return rc_m;
    }
    const float *d_depth = nullptr;
    {
        int rc_s = stage_depth(m, frame, &d_depth);  // once for all iterations
        if (rc_s) return rc_s;
        if ((rc_s = align::ensure_terms(m))) return rc_s;
        if ((rc_s = wait_for_input(m, m->stream))) return rc_s;
    }
    chisel_hip_align_result R;
    memset(&R, 0, sizeof(R));
    for (int i = 0; i < 12; i++) R.pose[i] = (double)frame->pose[i];
    R.status = CHISEL_HIP_ALIGN_ITERATION_LIMIT;
    int rc = CHISEL_HIP_OK;
    for (int it = 0; it < params->max_iterations; it++) {
        float pose_f[12];
        for (int i = 0; i < 12; i++) pose_f[i] = (float)R.pose[i];
        rc = align::launch_terms(m, frame, pose_f, d_depth, params->max_residual, m->align_mem.terms.get());
        if (rc) break;
        hipError_t e = hipMemcpyAsync(R.terms_last, m->align_mem.terms.get(), ALIGN_TERMS * sizeof(double), hipMemcpyDeviceToHost, m->stream);
        if (e == hipSuccess) e = wait_stream_spinning(m->stream);
        if (e != hipSuccess) {
            rc = fail(CHISEL_HIP_ERR_HIP, std::string("chisel_hip_align_depth: ") + hipGetErrorString(e));
            break;
        }
        if (it == 0) memcpy(R.terms_first, R.terms_last, sizeof(R.terms_first));
        if (R.terms_last[28] < (double)params->min_pixels) {
            R.status = CHISEL_HIP_ALIGN_TOO_FEW_PIXELS;
            break;
        }
        double xi[6];
        if (!align::solve(R.terms_last, params->damping, xi)) {
            R.status = CHISEL_HIP_ALIGN_DEGENERATE;
            break;
        }
        align::apply(xi, R.pose);
        memcpy(R.xi_last, xi, sizeof(xi));
        R.iterations = it + 1;
        if (align::norm3(xi) < params->min_translation && align::norm3(xi + 3) < params->min_rotation) {
            R.status = CHISEL_HIP_ALIGN_CONVERGED;
            break;
        }
    }
    if (rc) {
        (void)hipStreamSynchronize(m->stream);  // (the caller's image may be freed on return)
        return rc;
    }
    *result = R;
    return CHISEL_HIP_OK;
}

}  // extern "C"
