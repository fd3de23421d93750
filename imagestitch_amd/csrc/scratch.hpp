// scratch.hpp — what the per-thread stages share of their host plumbing (DESIGN.md §8 "The stages' per-thread scratch"): the 256-byte
// carving of a device buffer, the grow-only pinned buffer, the scratch of a stage that uploads its tables (with its two ordering rules), the
// capture check, a caller's mat against what a call needs, staged rows back to a host mat, device counts to the host, and StagedMat: a
// caller's host-or-device mat as a call's kernels see it.  Internal; per_thread<T>() stays in pairwise.hpp.
#pragma once
#include <algorithm>
#include <cstring>

#include "isx_internal.hpp"

namespace isx {

inline size_t round256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
struct Bump {                            // offsets into one buffer, 256-byte aligned
    size_t at = 0;
    size_t take(size_t bytes) { const size_t o = at; at += round256(bytes); return o; }
};

// A pinned host buffer that only grows.  reserve: holds `bytes` afterwards; when it has to grow, the old buffer is freed first and `want`
// bytes (the caller's growth rule, >= bytes) are allocated.  Whoever may still read the old buffer is waited for BEFORE the call.
struct PinBuf {
    void* p = nullptr; size_t cap = 0;
    int reserve(size_t bytes, size_t want) {
        if (cap >= bytes) return ISX_OK;
        ISX_TRY(release());
        ISX_HIP(hipHostMalloc(&p, want, hipHostMallocDefault));
        cap = want;
        return ISX_OK;
    }
    int release() { if (p) { ISX_HIP(hipHostFree(p)); p = nullptr; cap = 0; } return ISX_OK; }
};

// The scratch of a stage that uploads its tables (isx_match_features, isx_find_homography, isx_estimate_cameras): a device buffer `work` whose head is the upload,
// a pinned buffer `pin` that the host fills and one hipMemcpyAsync sends.  A call is begin(), fill pin.p, upload(), its launches, ran(), and
// never synchronises host and device where every mat is a device mat.  Two rules make that sound, and they live here only:
//   1. `pin` is not rewritten (or freed) until the upload that read it has completed: upload() records `uploaded`; begin() and release()
//      wait for it on the host before they touch `pin`.
//   2. `work` is not reused from another stream until the last call's kernels are through with it: ran() records `done` on that call's
//      stream, and begin() makes a call on any other stream wait for it (hipStreamWaitEvent: the host does not wait).  One stream orders
//      its own calls; a work.reserve() that grows frees the old buffer with hipFree, which waits for the device.
// One instance per calling thread and stage (per_thread<T>()), so no lock.  Known limit, left as it is: the Voronoi finder's VrScratch has no
// such fence - two isx_voronoi_seam_find calls of one thread on two streams share its `work` unordered; a fence there would add an event wait
// to what a captured graph contains.
struct UploadScratch {
    DevBuf work; PinBuf pin;
    int device = -1;
    hipEvent_t uploaded = nullptr, done = nullptr;
    bool pending = false, has_run = false;      // an upload may still be reading `pin`; `done` was recorded, on `last`
    hipStream_t last = nullptr;
    int wait_upload() { if (pending) { ISX_HIP(hipEventSynchronize(uploaded)); pending = false; } return ISX_OK; }
    int release() {
        ISX_TRY(wait_upload());
        if (uploaded) { ISX_HIP(hipEventDestroy(uploaded)); uploaded = nullptr; }
        if (done) { ISX_HIP(hipEventDestroy(done)); done = nullptr; }
        has_run = false;
        ISX_TRY(pin.release());
        work.release();
        device = -1;
        return ISX_OK;
    }
    // in this order: what another device holds is released, the previous upload has left `pin`, both buffers hold their bytes (pin grows
    // to half as much again, 64 KiB at least), the events exist, st waits for a call that ran on another stream
    int begin(int dev, hipStream_t st, size_t work_bytes, size_t upload_bytes) {
        if (device != dev) { ISX_TRY(release()); device = dev; }
        ISX_TRY(wait_upload());
        ISX_TRY(work.reserve(work_bytes));
        ISX_TRY(pin.reserve(upload_bytes, std::max<size_t>(upload_bytes + upload_bytes / 2, 1u << 16)));
        if (!uploaded) ISX_HIP(hipEventCreateWithFlags(&uploaded, hipEventDisableTiming));
        if (!done) ISX_HIP(hipEventCreateWithFlags(&done, hipEventDisableTiming));
        if (has_run && last != st) ISX_HIP(hipStreamWaitEvent(st, done, 0));
        return ISX_OK;
    }
    int upload(hipStream_t st, size_t bytes) {      // the first `bytes` of pin to the head of work
        ISX_HIP(hipMemcpyAsync(work.p, pin.p, bytes, hipMemcpyHostToDevice, st));
        ISX_HIP(hipEventRecord(uploaded, st));
        pending = true;
        return ISX_OK;
    }
    int ran(hipStream_t st) { ISX_HIP(hipEventRecord(done, st)); last = st; has_run = true; return ISX_OK; }      // after the call's last launch
};

inline int is_capturing(hipStream_t st, bool& yes) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    ISX_HIP(hipStreamIsCapturing(st, &cs));
    yes = cs != hipStreamCaptureStatusNone;
    return ISX_OK;
}
// for the entries that cannot be captured at all; `why` says what they do that a capture cannot hold
inline int refuse_capture(hipStream_t st, const char* who, const char* why) {
    bool yes = false;
    ISX_TRY(is_capturing(st, yes));
    ISX_CHECK_ARG(!yes, ISX_ERR_STATE, "%s: the stream is capturing (%s)", who, why);
    return ISX_OK;
}

// `what` `index` is a mat of `type` with at least rows x cols elements, `align`-byte aligned in pointer and step, a host mat or one of
// `device`.  Null data and any step are fine where the check stops early:
// STOP_NO_ROW_WANTED: once the call needs no row (an output it will not write); STOP_NO_ROW_PRESENT: once the mat has no row (an input whose
// rows are a capacity: those it has must be readable, and wide enough even when rows == 0 - the columns check, which nothing else can fail)
enum MatCheckStop { STOP_NO_ROW_WANTED, STOP_NO_ROW_PRESENT };
inline int check_mat_holds(const isx_mat& m, int type, long long rows, int cols, int align, MatCheckStop stop, int device, const char* who, const char* what,
                           int index) {
    ISX_CHECK_ARG(m.type == type, ISX_ERR_TYPE, "%s: %s %d is %s (%s)", who, what, index, type_name(m.type), type_name(type));
    ISX_CHECK_ARG(m.rows >= rows && (rows == 0 || m.cols >= cols), ISX_ERR_SIZE, "%s: %s %d is %d x %d, the call needs %lld x %d", who, what, index,
                  m.rows, m.cols, rows, cols);
    if (stop == STOP_NO_ROW_WANTED ? rows == 0 : m.rows == 0) return ISX_OK;
    ISX_CHECK_ARG(m.cols >= cols, ISX_ERR_SIZE, "%s: %s %d has %d columns, the call needs %d", who, what, index, m.cols, cols);
    ISX_CHECK_ARG(m.data != nullptr, ISX_ERR_INVALID, "%s: %s %d has a null data pointer", who, what, index);
    ISX_CHECK_ARG(m.step >= (size_t)m.cols * mat_elem_size(type) || m.rows == 1, ISX_ERR_INVALID, "%s: %s %d: step %zu smaller than a row", who, what, index, m.step);
    ISX_CHECK_ARG(((uintptr_t)m.data & (uintptr_t)(align - 1)) == 0 && (m.step & (size_t)(align - 1)) == 0, ISX_ERR_INVALID,
                  "%s: %s %d is not %d-byte aligned in pointer and step", who, what, index, align);
    ISX_CHECK_ARG(m.device < 0 || m.device == device, ISX_ERR_INVALID, "%s: %s %d lives on device %d, the call runs on %d", who, what, index, m.device, device);
    return ISX_OK;
}

// rows [0, rows) of a host mat, row_bytes each, back from their dense staged copy on the device (one row: whatever its step says)
inline int copy_rows_back(const isx_mat& m, const void* staged, long long rows, size_t row_bytes, hipStream_t st) {
    if (rows <= 0) return ISX_OK;
    if (rows == 1) ISX_HIP(hipMemcpyAsync(m.data, staged, row_bytes, hipMemcpyDeviceToHost, st));
    else ISX_HIP(hipMemcpy2DAsync(m.data, m.step, staged, row_bytes, row_bytes, (size_t)rows, hipMemcpyDeviceToHost, st));
    return ISX_OK;
}

// n counts (ints) of a device array on the host, complete on return: a stage reads them before it copies home the rows they name
inline int counts_to_host(int* host, const int* device_counts, int n, hipStream_t st) {
    ISX_HIP(hipMemcpyAsync(host, device_counts, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    ISX_HIP(hipStreamSynchronize(st));
    return ISX_OK;
}

// A caller's mat as one call's kernels see it.  A device mat is the mat itself.  A host mat is `staged`: a dense copy of its first `rows`
// rows, `row_bytes` each, inside the stage's `work` - an input in the upload (filled in `pin`), an output behind it (copied home after the
// launches).  plan() is the one place that says the row width: the space taken, the step the kernels are told and the bytes copied home all
// come from it.  An input is planned before upload_bytes is read off the Bump, an output after.  A mat of no rows is never staged, and
// nothing reads or writes it.  A 1 x n mat may be planned as one row of n elements.
struct StagedMat {
    const isx_mat* mat = nullptr;
    size_t row_bytes = 0, off = 0;       // off: of the staged copy in `work`, and in `pin`
    long long rows = 0;
    bool staged = false;
    void plan(Bump& lay, const isx_mat& m, long long rows_, size_t row_bytes_) {
        mat = &m; rows = rows_; row_bytes = row_bytes_;
        staged = m.device < 0 && rows > 0;
        if (staged) off = lay.take((size_t)rows * row_bytes);
    }
    template <class T>
    void bind(char* dev, T*& ptr) const { ptr = (T*)(staged ? dev + off : (char*)mat->data); }
    template <class T>
    void bind(char* dev, T*& ptr, long long& step) const { bind(dev, ptr); step = staged ? (long long)row_bytes : (long long)mat->step; }
    void fill(char* pin) const {         // an input's rows into the upload
        if (!staged) return;
        for (long long r = 0; r < rows; ++r) std::memcpy(pin + off + (size_t)r * row_bytes, (const char*)mat->data + (size_t)r * mat->step, row_bytes);
    }
    int back(const char* dev, long long n, hipStream_t st) const {      // an output's rows [0, n) home
        return staged ? copy_rows_back(*mat, dev + off, n, row_bytes, st) : ISX_OK;
    }
};

}  // namespace isx
