// filter_host.cpp -- the host skeleton of the lane-per-record filters (filter_host.hpp)
#include "filter_host.hpp"

namespace flbgpu {

std::string hexs(const std::string &s) {
    static const char *hx = "0123456789abcdef";
    std::string o;
    for (unsigned char c : s) { o.push_back(hx[c >> 4]); o.push_back(hx[c & 15]); }
    return o;
}

bool bad_args(int nprops, const char *const *names, const char *const *values) { return nprops < 0 || (nprops > 0 && (!names || !values)); }

void put_desc(char *desc, size_t cap, const std::string &text) {
    if (!desc || !cap) return;
    const size_t n = text.size() < cap - 1 ? text.size() : cap - 1;
    memcpy(desc, text.data(), n);
    desc[n] = 0;
}

bool upload(DevBuf &b, const void *src, size_t bytes) {
    if (!b.ensure(bytes + 16)) return false;
    if (bytes) HIPOK(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
    return true;
}

bool ensure_row_columns(flbgpu_filter *f, uint64_t n) {
    return f->d_len.ensure(n * sizeof(uint32_t)) && f->d_off.ensure((n + 1) * sizeof(uint64_t)) && f->d_scan_tmp.ensure(scan_tmp_elems(n) * sizeof(uint64_t));
}

bool scan_lengths_queue(flbgpu_filter *f, hipStream_t st, const uint32_t *len, uint64_t n, uint64_t *total) {
    { ProfScope ps(f, st, "k_scan"); launch_scan(len, n, f->d_scan_tmp.as<uint64_t>(), f->d_off.as<uint64_t>(), st, nullptr); }
    HIPOK(hipMemcpyAsync(total, f->d_off.as<uint64_t>() + n, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    return true;
}

bool scan_lengths_wait(flbgpu_filter *f, hipStream_t st, const uint64_t *total) {
    HIPOK(hipStreamSynchronize(st));
    return f->d_out.ensure(*total + 16);
}

void set_out(const flbgpu_filter *bytes_of, const flbgpu_filter *offsets_of, flbgpu_dev_chunk *out, uint64_t n, uint64_t total) {
    out->data = bytes_of->d_out.p; out->row_off = offsets_of->d_off.as<uint64_t>(); out->n = n; out->bytes = total;
}
void set_out(flbgpu_filter *f, flbgpu_dev_chunk *out, uint64_t n, uint64_t total) { set_out(f, f, out, n, total); }

// the most blocks a lane-per-record launch gets (lane_rows.inc): 65536.  The test switch FLBGPU_LANE_MAX_BLOCKS=<1 ... 65536>, read
// once per process, lowers it, so that the row loops' further trips are met with a thousand records; anything else leaves 65536.
unsigned lane_max_blocks() {
    static const unsigned cap = [] {
        const char *e = getenv("FLBGPU_LANE_MAX_BLOCKS");
        char *end = nullptr;
        const long v = e ? strtol(e, &end, 10) : 0;
        return (e && end != e && *end == 0 && v >= 1 && v <= 65536) ? (unsigned) v : 65536u;
    }();
    return cap;
}

}  // namespace flbgpu

extern "C" unsigned flbgpu_lane_max_blocks(void) { return flbgpu::lane_max_blocks(); }
