// pgmg_postpre_f32.hip — k_postpre_lds and its launchers (pgmg_postpre_impl.h) for float.
#include "pgmg_postpre_impl.h"

namespace pgmg {
PGMG_POSTPRE_INSTANTIATE(float)
}
