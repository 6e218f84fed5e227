// filter_host.hpp -- the host skeleton the lane-per-record filters share (modify.cpp, recmod.cpp, nest.cpp, typeconv.cpp, rtag.cpp,
// mlfilter.cpp, checklist.cpp): the front of parse_check / create, the upload of a program's tables, the counter words of one call with
// their round trip, and the tail that turns a length column into an output chunk.  What a filter DOES with its counters -- which one
// means "4 GB", when the call answers NOTOUCH, what `garbage` changes -- stays in its own file, next to its reference line numbers.
#pragma once
#include "host_int.hpp"

namespace flbgpu {

std::string hexs(const std::string &s);
bool bad_args(int nprops, const char *const *names, const char *const *values);
// the description of a checked program into the caller's buffer: cut to cap - 1 bytes, always terminated
void put_desc(char *desc, size_t cap, const std::string &text);
// b = the bytes, with 16 bytes of slack behind them (an empty table still has an address); nothing is copied when there are none
bool upload(DevBuf &b, const void *src, size_t bytes);
template <class T> bool upload(DevBuf &b, const std::vector<T> &v) { return upload(b, v.data(), v.size() * sizeof(T)); }

// The common front of flbgpu_<name>_parse_check and flbgpu_filter_<name>_create: the arguments, then parse(why).  false: refused, and
// flbgpu_last_error() reads "filter_<name>: <why>".
template <class Parse> bool parse_front(const char *name, int nprops, const char *const *names, const char *const *values, Parse parse) {
    std::string why;
    if (bad_args(nprops, names, values)) why = "bad arguments";
    else if (parse(why)) return true;
    set_err("filter_%s: %s", name, why.c_str());
    return false;
}

// the state of filter f when it is of this kind, else nullptr (the C ABI's accessors take any handle)
template <class S> S *state_of(flbgpu_filter *f, int kind) { return f && f->kind == kind ? static_cast<S *>(f->state) : nullptr; }

// One call's counter words: the words the kernels count into (W, on the device, `dev_extra` bytes behind them for a filter that keeps
// more there), their pinned host copy, and behind that copy the pinned totals (T) the scans' last elements are read into.
template <class W, class T = uint64_t> struct CallWords {
    ScopedDevBuf d;
    ScopedPinnedBuf h;
    bool ensure(size_t dev_extra = 0) { return d.ensure(sizeof(W) + dev_extra) && h.ensure(sizeof(W) + sizeof(T)); }
    W *dev() const { return d.as<W>(); }
    W &host() const { return *h.as<W>(); }
    T &total() const { return *(T *) (h.as<uint8_t>() + sizeof(W)); }
    // one counting pass: reset(host words) -> host to device -> launch() under a ProfScope -> device to host -> sync
    template <class Reset, class Launch> bool pass(flbgpu_filter *f, hipStream_t st, const char *prof_name, Reset reset, Launch launch) {
        reset(host());
        HIPOK(hipMemcpyAsync(dev(), &host(), sizeof(W), hipMemcpyHostToDevice, st));
        { ProfScope ps(f, st, prof_name); launch(); }
        HIPOK(hipMemcpyAsync(&host(), dev(), sizeof(W), hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        return true;
    }
};

// the columns every size / emit pair works on: f->d_len (n lengths), f->d_off (n + 1 offsets) and the scan's scratch
bool ensure_row_columns(flbgpu_filter *f, uint64_t n);
// The emit tail.  scan_lengths_queue: k_scan over len[0..n) into f->d_off, and d_off[n] on its way into *total (pinned).
// scan_lengths_wait: the sync -- behind whatever else the caller has queued for the same sync -- and f->d_out large enough for
// `total` bytes.  scan_lengths: the two in a row.
bool scan_lengths_queue(flbgpu_filter *f, hipStream_t st, const uint32_t *len, uint64_t n, uint64_t *total);
bool scan_lengths_wait(flbgpu_filter *f, hipStream_t st, const uint64_t *total);
inline bool scan_lengths(flbgpu_filter *f, hipStream_t st, const uint32_t *len, uint64_t n, uint64_t *total) {
    return scan_lengths_queue(f, st, len, n, total) && scan_lengths_wait(f, st, total);
}
// the output chunk of a call that emitted: f->d_out under the offsets of f->d_off
void set_out(flbgpu_filter *f, flbgpu_dev_chunk *out, uint64_t n, uint64_t total);
// ... of a pair that ran as one pass: the bytes are one filter's d_out, the offsets the other's d_off
void set_out(const flbgpu_filter *bytes_of, const flbgpu_filter *offsets_of, flbgpu_dev_chunk *out, uint64_t n, uint64_t total);

}  // namespace flbgpu
