"""DevBuf, the owner of the context's device buffers (prt_amd/csrc/prt_devbuf.h), against a counting allocator on the CPU:
tests/devbuf_main.cpp under AddressSanitizer and UBSan, as a program of its own (nothing of it is loaded into Python)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_devbuf_contract(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "devbuf_main")
    # the sanitizers' runtimes are linked statically: the program is complete in itself, whatever else the process environment loads
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include",
                           os.path.join(HERE, "devbuf_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "devbuf ok" in r.stdout
    assert r.stderr == "", r.stderr  # the sanitizers report nothing (a leak at exit would be reported here)
