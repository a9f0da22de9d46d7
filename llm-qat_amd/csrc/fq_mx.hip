// fq_mx.hip -- instantiations of the MX block-scaled fake quantization (fq_mx.h) for the three element types: a translation unit of its
// own, so the other units compile exactly as before.
#include "fq_mx.h"
namespace fq {
FQ_INSTANTIATE_MX(F32)
FQ_INSTANTIATE_MX(BF16)
FQ_INSTANTIATE_MX(F16)
}
