"""The environment maps the scene-edit tests build their tables from, on the host (tests/test_scene_edit_cpu.py) and on the device
(tests/test_gpu_scene_edit.py)."""
import prt_testlib as T

# width x height of the maps the GPU suite builds on the device as well (tests/test_gpu_scene_edit.py): one texel, one column, one row,
# more rows than a wavefront has lanes with a width that is no multiple of 64, more than two chunks per row
ENV_SHAPES = [(1, 1), (1, 7), (67, 1), (67, 70), (130, 3)]


def env_of(name):
    if name == "black_row":
        e = T.sky_env(64, 32)
        e[5, :, :3] = 0.0
        return e
    w, h = name
    return T.sky_env(w, h, seed=w + 100 * h)
