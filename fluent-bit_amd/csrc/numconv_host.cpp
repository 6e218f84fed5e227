// numconv_host.cpp -- host instantiation of numconv.hpp (diagnostic entry points: the CPU tests fuzz
// these against glibc; the kernels use the device instantiation of the same header).
#include "numconv.hpp"
#include <string.h>

namespace flbgpu { namespace nc {
const uint64_t g_pow5_host[2 * (P5_QMAX - P5_QMIN + 1)] = {
#include "pow5_table.inc"
};
struct PtrSrc { const uint8_t *p; uint32_t operator[](uint32_t i) const { return p[i]; } };
struct BufDst { char *p; int n; void put(uint32_t c) { p[n++] = (char) c; } };
}}

using namespace flbgpu::nc;

extern "C" {
int flbgpu_nc_scan_double(const char *s, int len, int mode, int exact, double *out, int *consumed) {
    PtrSrc src{(const uint8_t *) s};
    ScanResult r = exact ? scan_double<true>(src, (uint32_t) len, mode) : scan_double<false>(src, (uint32_t) len, mode);
    if (out) memcpy(out, &r.bits, 8);
    if (consumed) *consumed = (int) r.consumed;
    return r.status;
}
int flbgpu_nc_fmt_f6(double v, char *buf, int cap) {
    uint64_t bits;
    memcpy(&bits, &v, 8);
    BufDst d{buf, 0};
    return fmt_f6(bits, d, cap);
}
int flbgpu_nc_fmt_json_double(double v, int nan_to_null, char *buf) {
    uint64_t bits;
    memcpy(&bits, &v, 8);
    BufDst d{buf, 0};
    return fmt_json_double(bits, nan_to_null != 0, d);
}
// strtoimax (is_signed) / strtoumax over s[0 .. len), base 10 or 16: the 64 bits of the answer
unsigned long long flbgpu_nc_scan_intmax(const char *s, int len, int base, int is_signed) {
    PtrSrc src{(const uint8_t *) s};
    return scan_intmax(src, (uint32_t) len, (uint32_t) base, is_signed != 0);
}
int flbgpu_nc_fmt_lu(unsigned long long v, char *buf) {
    BufDst d{buf, 0};
    return fmt_lu((uint64_t) v, d);
}
// (double) of an integer, (int64_t) / (uint64_t) of a double as x86-64 answers; *undef is set where C leaves it undefined
double flbgpu_nc_int_to_double(unsigned long long v, int is_signed) {
    const uint64_t bits = is_signed ? i64_to_double_bits((int64_t) v) : u64_to_double_bits((uint64_t) v);
    double d;
    memcpy(&d, &bits, 8);
    return d;
}
unsigned long long flbgpu_nc_double_to_int(double v, int is_signed, int *undef) {
    uint64_t bits;
    memcpy(&bits, &v, 8);
    bool u = false;
    const uint64_t r = is_signed ? double_to_i64_x86(bits, u) : double_to_u64_x86(bits, u);
    if (undef) *undef = u ? 1 : 0;
    return r;
}
int flbgpu_nc_fmt_ld(long long v, char *buf) {
    BufDst d{buf, 0};
    return fmt_ld((int64_t) v, d);
}
}
