// Torch bindings for the defer_amd gfx950 kernel library.
//
// Host only. The entry points check device, dtype and contiguity and call
// the launchers of the .hip units on the current HIP stream, so ops compose
// with torch.cuda streams and hipGraph capture. They live in one entry_*.cpp
// per kernel family over the shared checks of entry_util.h.
#include "entry_util.h"

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    bind_conv(m);
    bind_dwconv(m);
    bind_pointwise(m);
    bind_attention(m);
    bind_fp8(m);
    bind_codec(m);
}
