// The tile kernels of the weight gradients as ONE translation unit: a family and its launcher live in a file of their own
// (wgrad_staged.hip, wgrad_multi.hip, wgrad_dma.hip), but the compiler optimises the device functions they share (wgrad_dev.h)
// across all their callers before it inlines them - compiled apart, the register-staged kernels come out with other instructions.
#include "wgrad_staged.hip"
#include "wgrad_multi.hip"
#include "wgrad_dma.hip"
