"""Host-only checks of `mdgen_amd.solver.resolve_solver`, the one place that turns (checkpoint's sampling_method, sampling_method,
num_steps, atol, rtol, sde, path_type) into a solver choice or an MdgenError, and of its use by `NewMDGenWrapper.inference()`,
`upsample()` and `rollout()`.  The wrapper is not constructed (its model needs a device): an instance made with `__new__` carries the
checkpoint args alone, and the batch it is handed fails the test when anything reads it."""
import argparse
import itertools

import pytest

REFUSED = "refused"
# (kind, steps) per sampling_method and num_steps (None / 1) on an Euler checkpoint with sde=None: what inference() did with these
# arguments before the resolver existed (its if-chain over dopri5 / SDE / RK / Euler and the defaults written in it).
TABLE = {
    None:       {None: ("euler", 49),    1: ("euler", 1)},
    "euler":    {None: ("euler", 49),    1: ("euler", 1)},
    "dopri5":   {None: ("dopri5", None), 1: REFUSED},          # num_steps sets the Euler grid; dopri5 chooses its own steps
    "midpoint": {None: ("rk", 24),       1: ("rk", 1)},
    "heun3":    {None: ("rk", 16),       1: ("rk", 1)},
    "rk4":      {None: ("rk", 12),       1: ("rk", 1)},
    "sde":      {None: ("sde", 49),      1: ("sde", 1)},
    "sde_heun": {None: ("sde", 49),      1: ("sde", 1)},
    "rk5":      {None: REFUSED,          1: REFUSED},          # not a solver
}
SDE_CASES = {"none": None, "empty": {}, "unknown_key": {"form": "sigma"}}


def expected(ckpt, method, num_steps, sde):
    """The other three axes on top of TABLE: num_steps 0 is refused everywhere; a non-Euler checkpoint is refused when neither a
    method nor num_steps is given; `sde` goes with the SDE methods only, and an unknown key of it is refused there too."""
    if num_steps == 0 or TABLE[method][num_steps] == REFUSED:
        return REFUSED
    if ckpt != "euler" and method is None and num_steps is None:
        return REFUSED
    if sde is not None and (method not in ("sde", "sde_heun") or sde):
        return REFUSED
    kind, steps = TABLE[method][num_steps]
    return kind, method or "euler", steps


CASES = list(itertools.product(("euler", "dopri5"), TABLE, (None, 1, 0), SDE_CASES))


def test_cases_are_the_whole_cross_product():
    assert len(CASES) == 2 * 9 * 3 * 3
    outcomes = [expected(c, m, n, SDE_CASES[s]) for c, m, n, s in CASES]
    assert sum(o != REFUSED for o in outcomes) == 37 and {o[0] for o in outcomes if o != REFUSED} == {"euler", "rk", "dopri5", "sde"}


@pytest.mark.parametrize("ckpt,method,num_steps,sde", CASES)
def test_resolver_table(ckpt, method, num_steps, sde):
    from mdgen_amd._lib import MdgenError
    from mdgen_amd.solver import resolve_solver
    want = expected(ckpt, method, num_steps, SDE_CASES[sde])
    if want == REFUSED:
        with pytest.raises(MdgenError):
            resolve_solver(ckpt, method, num_steps, 1e-6, 1e-3, SDE_CASES[sde], "GVP")
        return
    got = resolve_solver(ckpt, method, num_steps, 1e-5, 1e-2, SDE_CASES[sde], "GVP")
    assert (got.kind, got.method, got.steps) == want
    assert (got.atol, got.rtol) == (1e-5, 1e-2)
    if got.kind == "sde":   # the checked options: Euler-Maruyama / Heun, steps + 1 grid points, the wrapper's defaults
        o = got.sde_opts
        assert (o.method, o.n_points, o.diffusion_form, o.last_step) == (1 if method == "sde" else 2, got.steps + 1, 2, 1)
    else:
        assert got.sde_opts is None


def test_resolver_details():
    from mdgen_amd import wrapper
    from mdgen_amd._lib import MdgenError
    from mdgen_amd.solver import EULER_DEFAULT_STEPS, RK_DEFAULT_STEPS, SDE_DEFAULT_STEPS, SDE_DEFAULTS, SOLVERS, resolve_solver
    # the defaults stay importable from wrapper.py, and are the resolver's
    assert wrapper.RK_DEFAULT_STEPS is RK_DEFAULT_STEPS and wrapper.SDE_DEFAULTS is SDE_DEFAULTS
    assert wrapper.SDE_DEFAULT_STEPS == SDE_DEFAULT_STEPS == EULER_DEFAULT_STEPS == 49
    assert SOLVERS == ("euler", "dopri5", "midpoint", "heun3", "rk4", "sde", "sde_heun")
    # texts that callers and tests match, word for word
    with pytest.raises(MdgenError, match=r"sampling_method must be None, 'euler', 'dopri5', 'midpoint', 'heun3', 'rk4', 'sde' or "
                                         r"'sde_heun', got 'rk5'"):
        resolve_solver("euler", "rk5")
    with pytest.raises(MdgenError, match="num_steps sets the fixed Euler grid; dopri5 chooses its own steps"):
        resolve_solver("euler", "dopri5", 3)
    with pytest.raises(MdgenError, match=r"checkpoint args say sampling_method='dopri5'; pass sampling_method='dopri5' \(CLI"):
        resolve_solver("dopri5")
    with pytest.raises(MdgenError, match=r"sde options are \[.*\], got \['form'\]"):
        resolve_solver("euler", "sde", sde={"form": "sigma"})
    with pytest.raises(MdgenError, match="sde / noise are options of sampling_method='sde'"):
        resolve_solver("euler", "rk4", noise=object())
    # options of `sde` reach the library's struct; the path type is the checkpoint's
    o = resolve_solver("euler", "sde_heun", 4, sde=dict(last_step="Tweedie", diffusion_form="linear"), path_type="Linear").sde_opts
    assert (o.method, o.path, o.diffusion_form, o.last_step, o.n_points) == (2, 0, 3, 2, 5)
    with pytest.raises(MdgenError):   # a value the library refuses (SBDM needs sample_eps > 0)
        resolve_solver("euler", "sde", sde=dict(diffusion_form="SBDM"))


class _Untouchable(dict):
    """A batch that no refusal about solver arguments may read."""
    class Touched(Exception):
        pass

    def __getitem__(self, k):
        raise self.Touched(k)


def _wrapper(ckpt, cond_interval):
    from mdgen_amd.wrapper import NewMDGenWrapper
    w = NewMDGenWrapper.__new__(NewMDGenWrapper)
    w.args = argparse.Namespace(sampling_method=ckpt, path_type="GVP", tps_condition=False, sim_condition=True,
                                cond_interval=cond_interval, num_frames=8)
    return w


BAD = [("euler", dict(sampling_method="rk5")), ("euler", dict(sampling_method="dopri5", num_steps=3)), ("euler", dict(num_steps=0)),
       ("euler", dict(sampling_method="rk4", sde={})), ("euler", dict(sampling_method="sde", sde={"form": "sigma"})),
       ("euler", dict(sampling_method="sde_heun", sde=dict(diffusion_form="SBDM"))), ("dopri5", {})]


@pytest.mark.parametrize("ckpt,kw", BAD)
def test_the_three_call_sites_refuse_alike_before_touching_the_batch(ckpt, kw):
    from mdgen_amd._lib import MdgenError
    from mdgen_amd.solver import resolve_solver
    with pytest.raises(MdgenError) as want:
        resolve_solver(ckpt, kw.get("sampling_method"), kw.get("num_steps"), sde=kw.get("sde"))
    batch = _Untouchable()
    calls = (lambda: _wrapper(ckpt, None).inference(batch, **kw), lambda: _wrapper(ckpt, 4).upsample(batch, **kw),
             lambda: _wrapper(ckpt, None).rollout(batch, 8, 2, **kw))
    for call in calls:
        with pytest.raises(MdgenError) as got:
            call()
        assert str(got.value) == str(want.value)


def test_the_three_call_sites_go_on_to_the_batch_with_good_arguments():
    batch = _Untouchable()
    for kw in (dict(num_steps=3), dict(sampling_method="rk4"), dict(sampling_method="dopri5"), dict(sampling_method="sde", sde={})):
        for call in (lambda: _wrapper("dopri5", None).inference(batch, **kw), lambda: _wrapper("dopri5", 4).upsample(batch, **kw),
                     lambda: _wrapper("dopri5", None).rollout(batch, 8, 2, **kw)):
            with pytest.raises(_Untouchable.Touched):
                call()
