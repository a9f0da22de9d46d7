// fq_mx_cols.hip -- instantiations of the column-block MX fake quantization (fq_mx_cols.h) for the three element types.  A translation
// unit of its own: its 6 kernels are listed and compared (tools/isa_diff.py) apart from the row unit's 57 and the stochastic unit's 12.
#include "fq_mx_cols.h"
namespace fq {
FQ_INSTANTIATE_MX_COLS(F32)
FQ_INSTANTIATE_MX_COLS(BF16)
FQ_INSTANTIATE_MX_COLS(F16)
}
