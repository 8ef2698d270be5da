"""Trajectory upsampling, the parts that need no device: the window rule of the CLI, its parser, and the argument checks of
`mdgen_prep_keyframes` that run before any HIP call."""
import ctypes

import numpy as np
import pytest


def _reference_rule(n_key, num_frames, cond_interval):
    """The reference's `split_batch` restated on index arrays: total frames = n_key * c, int(total / T) windows, int(T / c) key
    frames each, window i scattering key frames [i*K, (i+1)*K) into rows [::c] of a T-row array."""
    total_frames = n_key * cond_interval
    total_items = int(total_frames / num_frames)
    cond_frames = int(num_frames / cond_interval)
    keys = np.arange(n_key)
    taken = []
    for i in range(total_items):
        window = np.full(num_frames, -1)
        window[::cond_interval] = keys[i * cond_frames:(i + 1) * cond_frames]   # raises where the two lengths differ
        taken.append(window[window >= 0])
    return total_items, cond_frames, taken


@pytest.mark.parametrize("case", [((100, 1000, 100), (10, 10), 0), ((25, 12, 4), (8, 3), 1), ((2, 12, 4), (0, 3), 2)])
def test_split_windows_matches_the_reference_rule(case):
    from mdgen_amd.upsampling_inference import split_windows
    (n_key, T, c), want, dropped = case
    got = split_windows(n_key, T, c)
    assert got == want
    n_ref, k_ref, taken = _reference_rule(n_key, T, c)
    assert got == (n_ref, k_ref)
    n_windows, K = got
    assert n_key - n_windows * K == dropped
    for i, tk in enumerate(taken):   # window i takes key frames [iK, (i+1)K)
        assert list(tk) == list(range(i * K, (i + 1) * K))


def test_split_windows_refuses_a_window_that_is_no_multiple_of_the_interval():
    from mdgen_amd.upsampling_inference import split_windows
    with pytest.raises(ValueError, match="multiple"):
        split_windows(10, 10, 3)
    with pytest.raises(ValueError):   # ... as the reference's slice assignment does
        _reference_rule(10, 10, 3)
    with pytest.raises(ValueError):
        split_windows(10, 12, 0)


def test_parser_has_the_reference_flags_with_its_defaults():
    from mdgen_amd.upsampling_inference import build_parser, parse_args
    a = build_parser().parse_args(["--data_dir", "d"])
    assert (a.ckpt, a.data_dir, a.suffix, a.pdb_id, a.batch_size, a.out_dir, a.split) == \
        (None, "d", "_i100", [], 1, ".", "splits/4AA_implicit_test.csv")
    assert (a.num_steps, a.sampling_method, a.precision, a.npy, a.xtc, a.synthetic) == (None, None, "bf16", False, False, False)
    a = parse_args(["--data_dir", "d", "--ckpt", "c.ckpt", "--pdb_id", "AAAA", "BBBB", "--batch_size", "16"])
    assert a.pdb_id == ["AAAA", "BBBB"] and a.batch_size == 16 and a.ckpt == "c.ckpt"
    a = parse_args(["--data_dir", "d", "--synthetic", "--num_frames", "12", "--cond_interval", "4"])
    assert (a.num_frames, a.cond_interval) == (12, 4)
    with pytest.raises(SystemExit):   # the Euler grid and the adaptive solver exclude each other
        parse_args(["--data_dir", "d", "--synthetic", "--num_steps", "3", "--sampling_method", "dopri5"])
    with pytest.raises(SystemExit):   # a checkpoint supplies num_frames / cond_interval itself
        parse_args(["--data_dir", "d", "--ckpt", "c.ckpt", "--num_frames", "12"])
    with pytest.raises(SystemExit):
        parse_args(["--data_dir", "d"])   # neither --ckpt nor --synthetic
    with pytest.raises(SystemExit):
        parse_args(["--synthetic"])       # --data_dir is required


def test_prep_keyframes_argument_validation_without_gpu():
    import mdgen_amd._lib as L
    sh = L.Shape(1, 8, 4)
    buf = ctypes.create_string_buffer(64)   # a non-null host address: the checks below return before anything reads it
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.lib.mdgen_prep_keyframes(ctypes.byref(sh), 4, None, p, p, p, p, p, p, None) == -1
    assert b"null" in L.lib.mdgen_last_error()
    assert L.lib.mdgen_prep_keyframes(None, 4, p, p, p, p, p, p, p, None) == -1
    assert L.lib.mdgen_prep_keyframes(ctypes.byref(sh), 0, p, p, p, p, p, p, p, None) == -2
    assert b"cond_interval" in L.lib.mdgen_last_error()
    bad = L.Shape(1, 0, 4)
    assert L.lib.mdgen_prep_keyframes(ctypes.byref(bad), 4, p, p, p, p, p, p, p, None) == -2


def test_upsample_euler_argument_validation_without_gpu():
    import mdgen_amd._lib as L
    sh = L.Shape(1, 8, 4)
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    tb = L.ResidueTables(*[p.value] * 8)
    args = [p] * 10
    # a null tensor; then cond_interval < 1: both before the context is looked at (it is null here) and before any HIP call
    assert L.lib.mdgen_upsample_euler(None, ctypes.byref(sh), 3, 4, None, *args[1:], ctypes.byref(tb), p, p, 0, 0, None) == -1
    assert L.lib.mdgen_upsample_euler(None, ctypes.byref(sh), 3, 0, *args, ctypes.byref(tb), p, p, 0, 0, None) == -2
    assert b"cond_interval" in L.lib.mdgen_last_error()
    assert L.lib.mdgen_upsample_euler(None, ctypes.byref(sh), 3, 4, *args, ctypes.byref(tb), p, p, 0, 0, None) == -1   # null context
