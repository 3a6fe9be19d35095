// The fused push of a set with deactivated streams (kws_stream_active.hip): the ACTIVE instantiations of kws_dscnn_fwd_kernel --
// F_STREAM | F_ACTIVE and F_STREAM | F_CLUSTER | F_ACTIVE, modes 4 and 5 -- with their launcher (launch_dscnn_stream_active) and
// their LDS opt-in (dscnn_active_init_device).  The kernel, its variant table and launch_variant are kws_dscnn.hip's, compiled
// here a second time with only these four rows in the table: a translation unit of their own keeps the compiler's decisions for
// the existing instantiations (inlining order, register allocation) exactly what they were without them.
#define KWS_DSCNN_ACTIVE_UNIT
#include "kws_dscnn.hip"
