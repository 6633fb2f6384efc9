#define UVS_PER_TRIAL
#define UVS_TU_NAME closed_grid_b
#define UVS_TU_METHODS UVS_METHOD_MCKF, UVS_METHOD_IMCCKF
#include "tu_closed_tuned.inc"
