"""DevEvent, HostBuf and StageTimer, the owners of the library's events and pinned memory and the scaffold of its profile calls
(prt_amd/csrc/prt_devres.h), against counting fakes on the CPU: tests/devres_main.cpp under AddressSanitizer and UBSan, as a program
of its own (nothing of it is loaded into Python).  Also the rule the header stands for: no raw event or pinned-memory call elsewhere."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "prt_amd", "csrc")


def test_devres_contract(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "devres_main")
    # the sanitizers' runtimes are linked statically: the program is complete in itself, whatever else the process environment loads
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include",
                           os.path.join(HERE, "devres_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "devres ok" in r.stdout
    assert r.stderr == "", r.stderr  # the sanitizers report nothing (a leaked event or pinned buffer would be reported here)


def test_raw_event_and_pinned_calls_live_in_one_header():
    allowed = {"hipEventCreate": {"prt_devres.h"}, "hipEventDestroy": {"prt_devres.h"}, "hipHostMalloc": {"prt_devres.h"},
               "hipHostFree": {"prt_devres.h"}, "hipEventElapsedTime": {"prt_devres.h", "prt_context.hip"}}
    for dirpath, _, files in os.walk(CSRC):
        for name in files:
            text = open(os.path.join(dirpath, name), errors="replace").read()
            for call, where in allowed.items():
                assert name in where or call not in text, f"{call} in {name}: events and pinned memory are owned by the types of prt_devres.h"
            if name not in ("prt_devres.h",):
                # a bare event array threaded through a queue function: only the timing ring's pair and BatchLaunch hand events out
                for line in text.splitlines():
                    if re.search(r"hipEvent_t\s*\*", line):
                        assert "prt_timing_pair" in line, f"{name}: {line.strip()}"
    context = open(os.path.join(CSRC, "prt_context.hip")).read()
    assert context.count("hipEventElapsedTime") == 1 and "hipEventElapsedTime" in context[context.index("fold_timing"):context.index("prt_timing_pair(prt_hip_ctx")]
