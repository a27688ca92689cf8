"""PrtIoArray and PrtStage, the array table and the one staging arena of the host-array entry points (prt_amd/csrc/prt_stage.h),
against fakes that copy and log on the CPU: tests/stage_main.cpp under AddressSanitizer and UBSan, as a program of its own (nothing of
it is loaded into Python).  Also the rule the header stands for: no family of entry points keeps a staged path of its own."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "prt_amd", "csrc")

# the per-family staging members the arena replaced
OLD_MEMBERS = ["qRays", "qHits", "qSurf", "qOccl", "qRad", "bkPoints", "bkDirs", "bkWeights", "bkOut", "atUV", "atTexels", "atHits", "atPoints",
               "atValues", "atImage", "atMask"]


def test_stage_contract(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "stage_main")
    # the sanitizers' runtimes are linked statically: the program is complete in itself, whatever else the process environment loads
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include",
                           os.path.join(HERE, "stage_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "stage ok" in r.stdout
    assert r.stderr == "", r.stderr  # the sanitizers report nothing (a copy past a slice or a leaked arena would be reported here)


def test_host_arrays_are_staged_in_one_place():
    sources = {}
    for dirpath, _, files in os.walk(CSRC):
        for name in files:
            sources[name] = open(os.path.join(dirpath, name), errors="replace").read()
    for name, text in sources.items():
        # the flag and a stream copy in one file: a staged path.  Only the arena and the call path that drives it may have both
        if name not in ("prt_stage.h", "prt_context.hip"):
            assert not ("PRT_HIP_QUERY_HOST" in text and "hipMemcpyAsync" in text), f"{name} stages host arrays of its own"
        if name != "prt_context.hip":
            code = "\n".join(line.split("//")[0] for line in text.splitlines())
            assert "PRT_HIP_QUERY_HOST" not in code, f"{name} branches on PRT_HIP_QUERY_HOST: prt_run_io does"
        assert not re.search(r"\w_(staged|direct)\b", text), f"{name}: a staged / direct pair"
        for member in OLD_MEMBERS:
            assert not re.search(rf"\b{member}\b", text), f"{name}: {member}, a staging buffer of one family"
    assert sum(len(re.findall(r"\bbool aligned\(", text)) for text in sources.values()) == 1
    assert sum(text.count('": unknown flag bits"') for text in sources.values()) == 1  # prt_check_flags
    # the arena is the context's one staging member, and every host-array entry point goes through the one call path
    assert len(re.findall(r"\bPrtStage\b", sources["prt_internal.h"])) == 1
    for name, calls in (("prt_query.hip", 2), ("prt_bake.hip", 1), ("prt_atlas.hip", 3)):
        assert sources[name].count("prt_run_io(") == calls, name
