// decode_stubs.cpp -- stand-ins for the 14 prt_hip_* calls host/prt_host.cpp refers to, so that tests/decode_main.cpp links without
// HIP.  The asset readers never reach the device: a call that arrives here is a bug, and ends the program.
#include <cstdlib>

#define STUB(name) \
    extern "C" int name() { abort(); }
STUB(prt_hip_build_bvh)
STUB(prt_hip_create)
STUB(prt_hip_destroy)
STUB(prt_hip_device_count)
STUB(prt_hip_display)
STUB(prt_hip_download)
STUB(prt_hip_download_display)
STUB(prt_hip_get_stats)
STUB(prt_hip_render)
STUB(prt_hip_render_gbuffer)
STUB(prt_hip_set_camera)
STUB(prt_hip_upload)
STUB(prt_hip_upload_scene)
extern "C" const char* prt_hip_last_error() { abort(); }
