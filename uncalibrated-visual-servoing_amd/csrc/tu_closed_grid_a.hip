#define UVS_PER_TRIAL
#define UVS_TU_GRID_NAME closed_grid_a
#define UVS_TU_GRID_METHODS UVS_METHOD_GMCKF, UVS_METHOD_KF
#include "tu_closed_grid.inc"
