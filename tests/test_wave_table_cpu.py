"""The wave table of the audio units (csrc/bm_wave.h) on the host: the entry, ``bm_wave_table_fill`` and the argument
checks of the four launchers over it.  Every call here returns ``BM_ERR_ARG`` before anything touches a device, so the
device pointers are placeholders."""
import ctypes

import numpy as np
import pytest

BM_ERR_ARG = 1001
PLACEHOLDER = ctypes.c_void_p(4096)          # non-null, 8-byte aligned, never dereferenced


@pytest.fixture(scope="module")
def L():
    from brainmagick_amd import _lib
    return _lib.lib()


def _lengths(*values):
    return np.ascontiguousarray(values, dtype=np.int64)


def _launchers(L):
    """name -> (call(lengths, n_waves), the L at the launcher's own lower bound)."""
    range_host = np.zeros((1, 2), dtype=np.int32)

    def ptr(a):
        return ctypes.c_void_p(a.ctypes.data)
    P = PLACEHOLDER
    return {
        "wave_moments": (lambda ln, n: L.bm_wave_moments(P, ptr(ln), n, P, P, 1, P, None), 0),
        "resample_frac": (lambda ln, n: L.bm_resample_frac(P, ptr(ln), n, None, P, 1, 2, 26, None), 0),
        "mel_spectrogram": (lambda ln, n: L.bm_mel_spectrogram(P, ptr(ln), n, None, P, 512, 272, P, P, ptr(range_host), 1, 1,
                                                               1e-5, None), 512 // 2),
        "yin_pitch": (lambda ln, n: L.bm_yin_pitch(P, ptr(ln), n, 16_000.0, 256, 64, 45, 160, 0.1, None), 256),
    }


def test_the_entry_is_24_bytes_and_fill_checks_it(L):
    assert L.bm_version() >= 116
    assert L.bm_wave_table_entry_bytes() == 24
    entry = np.zeros(24, dtype=np.uint8)
    e = ctypes.c_void_p(entry.ctypes.data)
    for args in ((None, PLACEHOLDER, 100, None),                             # a null entry
                 (e, None, 100, None),                                       # a null waveform
                 (e, PLACEHOLDER, 0, None),
                 (e, PLACEHOLDER, 2 ** 31, None),
                 (e, ctypes.c_void_p(4098), 100, None),                      # a waveform that is not 4-byte aligned
                 (e, PLACEHOLDER, 100, ctypes.c_void_p(4098))):              # an output that is not
        assert L.bm_wave_table_fill(*args) == BM_ERR_ARG, args
        assert L.bm_last_error().decode().startswith("wave table:")
    assert not entry.any()                                                   # a refused entry is left as it was
    assert L.bm_wave_table_fill(e, PLACEHOLDER, 2 ** 31 - 1, None) == 0
    assert entry.view(np.int64).tolist() == [4096, 0, 2 ** 31 - 1]           # {x, out, L}


@pytest.mark.parametrize("name", ["wave_moments", "resample_frac", "mel_spectrogram", "yin_pitch"])
def test_every_launcher_checks_the_table_before_it_launches(L, name):
    call, lower = _launchers(L)[name]
    for lengths, n_waves, word in ((_lengths(4000), 65536, "limit is 65535"),
                                   (_lengths(4000, 2 ** 31), 2, "waveform 1 has 2147483648 samples"),
                                   (_lengths(lower), 1, f"waveform 0 has {lower} samples")):
        assert call(lengths, n_waves) == BM_ERR_ARG, (lengths, n_waves)
        message = L.bm_last_error().decode()
        assert message.startswith(name + ":") and word in message, message


def test_resample_checks_the_output_length_too(L):
    call, _ = _launchers(L)["resample_frac"]
    assert call(_lengths(2 ** 31 - 1), 1) == BM_ERR_ARG                     # 1 Hz -> 2 Hz: 2^32 - 2 outputs
    message = L.bm_last_error().decode()
    assert message.startswith("resample_frac:") and "outputs" in message, message
