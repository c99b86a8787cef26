//  icm_internal.hh -- what the host classes of icm.hh share behind their public interface (not part of the drop-in header).

#ifndef GMG_HOST_ICM_INTERNAL_HH_INCLUDED
#define GMG_HOST_ICM_INTERNAL_HH_INCLUDED

#include <mutex>

struct gmg_single;   // include/gmg.h

namespace gmg_host {

//  A model's device mirror (ICM_t::dev_mirror, Fixed_Length_ICM_t::dev_fixed) is made at its first use by a const method, and
//  const methods of one model may run on several host threads: the first use and the drop of a mirror hold this lock (one for
//  all models: an upload happens once in a model's life), and the pointer is published / read with release / acquire order.
//  The members stay plain pointers: the class layout in icm.hh is the drop-in interface.
//  No path reaches exit () with the lock held, and a model without a mirror does not take it in its destructor: exit () runs the
//  destructors of models in static storage on the thread that failed (tests/test_host_fatal_exit.py).
std :: mutex  & Mirror_Mutex  (void);
template <class T>  T  * Mirror_Load  (T * const & slot)  { return  __atomic_load_n (& slot, __ATOMIC_ACQUIRE); }
template <class T>  void  Mirror_Store  (T * & slot, T * value)  { __atomic_store_n (& slot, value, __ATOMIC_RELEASE); }

//  "ERROR:  <who>: <gmg_last_error ()>" on stderr, then exit (EXIT_FAILURE): the reference's convention for a failed call
void  Device_Fatal  (const char * who);
//  gmg_init on device $GMG_DEVICE (default 0), once per process (std::call_once: whichever threads get here first)
void  Ensure_Device  (void);
//  the calling thread's one-string staging (include/gmg.h, gmg_single), made at its first use
gmg_single  * Thread_Staging  (void);

}  // namespace gmg_host

#endif
