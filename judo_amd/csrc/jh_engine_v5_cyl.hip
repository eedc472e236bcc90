// jh_engine_v5_cyl.hip -- the leap kernel (jh_engine_v5.hip) instantiated a third time: the 64-contact build (caltech_leap_cube ships with 64) with the cylinder narrow
// phases compiled in, for a model image that keeps the fingertip cylinders of the Caltech hand instead of their sphere stand-ins (engine_model.pack_engine_model,
// fingertips="cylinder").  A separate translation unit, as jh_engine_v5_cap64.hip is: the 48- and 64-contact builds compile to the code they had before, and
// jh_model_create selects this one for an image that holds a cylinder and for no other.
#define JH_V5_NSBIG 4
#define JH_V5_CYL 1
#define JH_V5_NAME(f) f##_cyl
#include "jh_engine_v5.hip"
