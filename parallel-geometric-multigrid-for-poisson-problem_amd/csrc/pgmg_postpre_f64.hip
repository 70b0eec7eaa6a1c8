// pgmg_postpre_f64.hip — k_postpre_lds and its launchers (pgmg_postpre_impl.h) for double.
#include "pgmg_postpre_impl.h"

namespace pgmg {
PGMG_POSTPRE_INSTANTIATE(double)
}
