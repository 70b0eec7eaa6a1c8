// pgmg_postpre_f64s.hip — the sampled-check forms of k_postpre_lds (pgmg_postpre_impl.h) for
// double (16 kernel instantiations).
#define PGMG_POSTPRE_SAMPLED_TU
#include "pgmg_postpre_impl.h"

namespace pgmg {
PGMG_POSTPRE_SAMPLED_INSTANTIATE(double)
}
