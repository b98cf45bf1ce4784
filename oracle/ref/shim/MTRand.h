/* Case-sensitive file systems: the reference includes its Mersenne twister header under this spelling. */
#include "mtrand.h"
