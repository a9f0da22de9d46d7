// fq_mx_cols.hip -- instantiations of the column-block MX fake quantization (fq_mx_cols.h) for the three element types: a translation
// unit of its own, so the other units compile exactly as before.
#include "fq_mx_cols.h"
namespace fq {
FQ_INSTANTIATE_MX_COLS(F32)
FQ_INSTANTIATE_MX_COLS(BF16)
FQ_INSTANTIATE_MX_COLS(F16)
}
