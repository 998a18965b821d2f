/* Stand-in for <cuda.h>: the host build of the reference needs nothing from it. */
#pragma once
