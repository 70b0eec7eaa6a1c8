// pgmg_postpre_f32s.hip — the sampled-check forms of k_postpre_lds (pgmg_postpre_impl.h) for
// float (8 kernel instantiations).
#define PGMG_POSTPRE_SAMPLED_TU
#include "pgmg_postpre_impl.h"

namespace pgmg {
PGMG_POSTPRE_SAMPLED_INSTANTIATE(float)
}
