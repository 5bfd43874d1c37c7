// host_totals.h -- the frame of the entries that wait ONCE for a few totals (included by chisel_hip.hip in front of them).  Such an
// entry reads top to bottom: refusals, the inputs (host arrays are staged through one owned device buffer), the scratch the map owns
// (grown on demand, freed with the map), its kernels on the map's stream behind what was queued before, THE WAIT for the totals in
// pinned memory -- alone for the coarse and the indexed mesh, whose scan kernels write them, behind the report kernel of a ControlWords
// (host_buffer.h) for the mesh components, the adjacency passes and the frontiers --, the capacities, then what writes the caller's
// arrays: with device pointers nothing is waited for behind those launches; host arrays are staged through a second owned buffer
// sized by the totals, copied out once with exactly their live rows, and are complete on return.
#pragma once

namespace {

// null map, a group, then the device: the entries that run on one device and one stream and neither read nor write the map
int begin_on_one_device(chisel_hip_map *m, const char *name) {
    if (!m) return fail(CHISEL_HIP_ERR_INVALID, "null map");
    if (m->is_group) return fail(CHISEL_HIP_ERR_UNSUPPORTED, std::string(name) + " runs on one device and one stream: a group has several (hand it a map of one shard)");
    HIP_TRY(hipSetDevice(m->device));
    return CHISEL_HIP_OK;
}

int refusal(const char *name, const char *why, bool unsupported) { return fail(unsupported ? CHISEL_HIP_ERR_UNSUPPORTED : CHISEL_HIP_ERR_INVALID, std::string(name) + ": " + why); }
int hip_failure(const char *name, hipError_t e) { return fail(CHISEL_HIP_ERR_HIP, std::string(name) + ": " + hipGetErrorString(e)); }

// a pass's scratch, carved out of one buffer of ints: at least `need`, doubled when it grows, never fewer than 4096
int grow_ints(chisel_hip_map *m, DeviceBuffer<int> &words, size_t need) {
    if (need <= words.size()) return CHISEL_HIP_OK;
    return grow_buffer(words, std::max<size_t>(std::max<size_t>(need, 2 * words.size()), 4096), m->stream);  // (waits for the stream before it replaces the buffer)
}

// THE WAIT of a call, behind the kernel that writes its totals into pinned memory: the launches are checked, the words complete
int wait_for_words(chisel_hip_map *m) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(m->stream));  // THE WAIT
    note_stream_idle(m);
    std::atomic_thread_fence(std::memory_order_acquire);
    return CHISEL_HIP_OK;
}

// The tail of a call whose table is host memory whatever on_device says: the `words` words a kernel behind the call's wait wrote into
// `table`, into out.  `e`: what Staging::finish said -- host arrays have waited there; device arrays are left on the stream, the table is not.
hipError_t read_pinned_table(chisel_hip_map *m, PinnedWords &table, size_t words, bool on_device, hipError_t e, int64_t *out) {
    if (e != hipSuccess) return e;
    if (on_device) e = hipStreamSynchronize(m->stream);
    std::atomic_thread_fence(std::memory_order_acquire);
    volatile long long *rows = table.get();
    for (size_t i = 0; e == hipSuccess && i < words; i++) out[i] = rows[i];
    return e;
}

}  // namespace

namespace chisel_hip {

inline int ControlWords::prepare(chisel_hip_map *m, size_t n) {
    if (!ctl_) HIP_TRY(ctl_.alloc(n));
    HIP_TRY(host_.ensure(n, m->stream));
    return CHISEL_HIP_OK;
}

inline int ControlWords::report_and_wait(chisel_hip_map *m, volatile long long **words) {
    hipLaunchKernelGGL(report_words_kernel<unsigned long long>, dim3(1), dim3(64), 0, m->stream, (const unsigned long long *)ctl_.get(), (unsigned long long *)host_.dev(),
                       (int)ctl_.size());
    *words = host_.get();
    return wait_for_words(m);
}

}  // namespace chisel_hip
