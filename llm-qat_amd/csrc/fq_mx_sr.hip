// fq_mx_sr.hip -- instantiations of the stochastic-rounding MX fake quantization (fq_mx_sr.h) for the three element types, and the host
// restatement of its noise index (fqs_mx_noise).  A translation unit of its own; it shares the stages of fq_mx.h and fq_mx_cols.h with
// fq_mx.hip and fq_mx_cols.hip, so a change to one of those headers is checked on all three listings.
#include "fq_mx_sr.h"
namespace fq {
FQ_INSTANTIATE_MX_SR(F32)
FQ_INSTANTIATE_MX_SR(BF16)
FQ_INSTANTIATE_MX_SR(F16)

// R16 of the flat elements first .. first + n - 1 of a tensor whose 16-byte vector holds epv elements, through the function the kernels call
void mx_sr_host_noise(MxSrKey k, int64_t first, int64_t n, int epv, uint16_t* out) {
    for (int64_t i = first; i < first + n; ++i) {
        const int64_t w = i / epv;
        const int e = (int)(i - w * epv);
        uint32_t word;
        if (epv == 8) {
            uint32_t rw[4];
            mx_sr_words<8>(w, k, rw);
            word = rw[e >> 1];
        } else {
            uint32_t rw[2];
            mx_sr_words<4>(w, k, rw);
            word = rw[e >> 1];
        }
        out[i - first] = (uint16_t)((e & 1) ? word >> 16 : word & 0xFFFFu);
    }
}
}
