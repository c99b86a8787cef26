//  icm_internal.hh -- what the host classes of icm.hh share behind their public interface (not part of the drop-in header).

#ifndef GMG_HOST_ICM_INTERNAL_HH_INCLUDED
#define GMG_HOST_ICM_INTERNAL_HH_INCLUDED

struct gmg_single;   // include/gmg.h

namespace gmg_host {

//  "ERROR:  <who>: <gmg_last_error ()>" on stderr, then exit (EXIT_FAILURE): the reference's convention for a failed call
void  Device_Fatal  (const char * who);
//  gmg_init on device $GMG_DEVICE (default 0), once per process
void  Ensure_Device  (void);
//  the calling thread's one-string staging (include/gmg.h, gmg_single), made at its first use
gmg_single  * Thread_Staging  (void);

}  // namespace gmg_host

#endif
