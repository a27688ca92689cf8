"""The display transform without a GPU: the arithmetic the kernels run (prt_amd/csrc/prt_display.h, on the host through
prt_hip_test_display_host) against the numpy restatement of the header (prt_display_ref) at tolerance 0, against the pixel block
prt_amd.save_ppm writes, and the generalised powf restatement of prt_devmath.h against libm."""
import ctypes as C
import itertools
import subprocess

import numpy as np
import pytest

import prt_amd
import prt_display_ref as R
import prt_testlib as T
from prt_display_ref import BAD_FIELDS, assert_state_equal, frame

P = prt_amd.DisplayParams.make
F = np.float32


@pytest.fixture(scope="module", autouse=True)
def built():
    prt_amd.build()


def state_struct(d):
    s = prt_amd.DisplayState(float(d["gain"]), int(d["valid"]), float(d["octaves"]), float(d["target"]), int(d["metered"]), int(d["ignored"]))
    s.hist[:] = [int(x) for x in d["hist"]]
    return s


def test_the_straddling_pairs_straddle():
    """The hostile image's threshold pairs are neighbouring floats whose bytes are v - 1 and v, for every v of both transfers."""
    for transfer in (0, 1):
        th = R.thresholds(transfer)
        assert (th.view(np.uint32)[:, 1] - th.view(np.uint32)[:, 0] == 1).all()
        b = R.channel_bytes(th, F(1), 0, transfer)
        assert np.array_equal(b[:, 1], np.arange(1, 256)) and np.array_equal(b[:, 0], np.arange(0, 255)), transfer


def test_host_arithmetic_equals_the_restatement_on_the_hostile_image():
    img = R.hostile_image()
    for tonemap, transfer, fmt in itertools.product((0, 1), (0, 1), (0, 1, 2)):
        for gain in (1.0, 0.37):
            p = P(tonemap=tonemap, transfer=transfer, format=fmt, gain=gain)
            got, _ = prt_amd.display_host(img, p)
            want, _ = R.display(img, p)
            assert np.array_equal(got, want), (tonemap, transfer, fmt, gain, int((got != want).sum()))
    # metered, a rectangle only: bytes outside it stay, the meter sees the rectangle alone
    p = P(tonemap=1, transfer=1, format=1, meter=True, gain=1.5, adapt_rate=1.0)
    base = np.full((37, 61, 4), 0xA5, np.uint8)
    got, st = prt_amd.display_host(img, p, x0=3, y0=5, x1=57, y1=30, out=base.copy())
    want, ws = R.display(img, p, x0=3, y0=5, x1=57, y1=30, out=base)
    assert np.array_equal(got, want)
    assert_state_equal(st, ws)
    assert ws["metered"] + ws["ignored"] == 55 * 26 and (got[:5] == 0xA5).all() and (got[:, :3] == 0xA5).all()


@pytest.mark.parametrize("tonemap", [True, False])
def test_transfer_0_gain_1_is_the_pixel_block_of_save_ppm(tmp_path, tonemap):
    img = R.hostile_image()
    path = tmp_path / "o.ppm"
    prt_amd.save_ppm(str(path), img, tonemap=tonemap)
    data = open(path, "rb").read()
    assert data.startswith(b"P6\n61 37\n255\n")
    block = np.frombuffer(data[-61 * 37 * 3:], np.uint8).reshape(37, 61, 3)
    got, _ = prt_amd.display_host(img, P(tonemap=tonemap, transfer=0, format=0, gain=1.0))
    assert np.array_equal(got, block), int((got != block).sum())


def test_generalised_powf_matches_libm_for_both_display_exponents(tmp_path):
    """prt_powf_pos(x, 1/2.2f) and (x, 1/2.4f) against the machine's powf: every float in [2^-24, 1], every 13th bit pattern below
    (subnormals and tiny normals), and 0."""
    src = tmp_path / "pw.c"
    src.write_text(r'''
#include <stdio.h>
#include <math.h>
#include <string.h>
#include "%s/prt_amd/csrc/prt_devmath.h"
static long check(uint32_t b, float e){ float x; memcpy(&x,&b,4); float m=prt_powf_pos(x,e), g=powf(x,e); return memcmp(&m,&g,4) != 0; }
int main(){ long bad=0; const float es[2] = {1/2.2f, 1/2.4f};
  for(int k=0;k<2;k++){
    for(uint32_t b=0x33800000u;b<=0x3f800000u;b++) bad += check(b, es[k]);
    for(uint32_t b=0;b<0x33800000u;b+=13) bad += check(b, es[k]);
  }
  printf("%%ld\n", bad); return 0; }
''' % T.ROOT)
    exe = tmp_path / "pw"
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-mfma", str(src), "-o", str(exe), "-lm"])
    assert subprocess.check_output([str(exe)]).decode().strip() == "0"


def test_metering_special_cases():
    p = P(meter=True, adapt_rate=0.25)
    # an all-black image (and black with NaN, negatives, -inf) leaves the state as it is
    prior = R.resolve(*R.histogram(frame(1.0, 1)), p, R.fresh_state())
    black = np.zeros((24, 40, 3), F)
    black[0, 0] = np.nan
    black[0, 1] = -1.0
    black[0, 2] = (-np.inf, 0, 0)
    _, st = prt_amd.display_host(black, p, state=state_struct(prior))
    assert_state_equal(st, prior, "all black")
    _, st = prt_amd.display_host(black, p)
    assert_state_equal(st, R.fresh_state(), "all black, fresh")
    # +inf lands in bin 255, NaN is ignored
    img = frame(1.0, 2)
    img[3, 3] = np.inf
    img[4, 4] = (np.inf, 0, 0)
    img[5, 5] = np.nan
    img[6, 6] = (1, np.nan, 1)
    img[7, 7] = 1e30
    _, st = prt_amd.display_host(img, p)
    d = st.as_dict()
    assert d["hist"][255] == 3 and d["ignored"] == 2 and d["metered"] == 24 * 40 - 2
    assert_state_equal(st, R.display(img, p)[1], "inf / nan")
    # low = 0, high = 1000 averages everything: the mean of 2k + 1 over every counted pixel
    q = P(meter=True, low_permille=0, high_permille=1000)
    _, st = prt_amd.display_host(img, q)
    d = st.as_dict()
    k = np.arange(256, dtype=np.uint64)
    S, N = int((d["hist"].astype(np.uint64) * (2 * k + 1)).sum()), int(d["hist"].sum())
    m = np.array([S], np.uint64).astype(F)[0] / np.array([N], np.uint64).astype(F)[0]
    assert d["octaves"].view(np.uint32) == (F(m * F(0.0625)) - F(16)).view(np.uint32) and N == d["metered"]
    assert_state_equal(st, R.display(img, q)[1], "whole band")


def test_adaptation_sequence_word_for_word():
    """Three frames of different brightness at adaptRate 0.25: the first jumps, the next two move a quarter of the way; at adaptRate 1
    the gain is the target exactly."""
    p = P(meter=True, adapt_rate=0.25, tonemap=1, transfer=1, format=2)
    st, ws = None, None
    gains = []
    for n, level in enumerate((1.0, 30.0, 0.02)):
        img = frame(level, 10 + n)
        got, st = prt_amd.display_host(img, p, state=st)
        want, ws = R.display(img, p, state=ws)
        assert np.array_equal(got, want), n
        assert_state_equal(st, ws, f"frame {n}")
        gains.append((F(st.gain), F(st.target)))
    assert gains[0][0] == gains[0][1] and gains[1][0] != gains[1][1] and gains[2][0] != gains[2][1]
    assert len({g.tobytes() for g, _ in gains}) == 3
    _, st1 = prt_amd.display_host(frame(5.0, 3), P(meter=True, adapt_rate=1.0), state=st)
    assert F(st1.gain).view(np.uint32) == F(st1.target).view(np.uint32) and st1.target != st.target
    # the clamps of the target
    _, lo = prt_amd.display_host(frame(1e4, 4), P(meter=True, min_gain=0.5, max_gain=2.0))
    _, hi = prt_amd.display_host(frame(1e-4, 5), P(meter=True, min_gain=0.5, max_gain=2.0))
    assert lo.gain == 0.5 and hi.gain == 2.0


def test_host_entry_refuses_every_field_by_name():
    img = frame(1.0, 7)
    for field, kw in BAD_FIELDS:
        with pytest.raises(prt_amd.PrtError) as e:
            prt_amd.display_host(img, P(**kw))
        assert "(-2)" in str(e.value) and field in str(e.value), (kw, str(e.value))
    with pytest.raises(prt_amd.PrtError, match="rectangle"):
        prt_amd.display_host(img, P(), x1=40)
    prt_amd.display_host(img, P(key=float("nan"), adapt_rate=7.0))  # the meter's fields are only read with meter 1


def test_struct_layouts_match_the_header():
    assert C.sizeof(prt_amd.DisplayParams) == 44 and C.sizeof(prt_amd.DisplayState) == 32 + 1024
    assert prt_amd.DisplayState.metered.offset == 16 and prt_amd.DisplayState.hist.offset == 32
