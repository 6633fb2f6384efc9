#define UVS_PER_TRIAL
#define UVS_TU_NAME closed_grid_a
#define UVS_TU_METHODS UVS_METHOD_GMCKF, UVS_METHOD_KF
#include "tu_closed_tuned.inc"
