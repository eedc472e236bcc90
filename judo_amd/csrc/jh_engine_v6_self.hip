// jh_engine_v6_self.hip -- the fr3_pick kernel (jh_engine_v6.hip) instantiated a second time, with every collision pair the MJCF leaves (fr3_components/fr3.xml:11-99:
// 190 after MuJoCo's static filters): on top of the default build's 78 the arm links against each other (22 capsule-capsule) and the hand / finger boxes against the link
// capsules, the static fr3_link0 included (90 box-capsule).  A contact between two arm bodies is a general contact whose Jacobian is the deeper body's columns below the
// shallower body's depth (slot_sides).  A separate translation unit, as jh_engine_v5_cyl.hip is: the default build compiles to the code it had, and jh_model_create selects
// this one for an image that holds such a pair (engine_model.pack_engine_model on a description with "self_collision": FR3Pick(self_collision=True)) and for no other.
#define JH_V6_SELF 1
#define JH_V6_NAME(f) f##_self
#include "jh_engine_v6.hip"
