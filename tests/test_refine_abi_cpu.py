"""CPU: the refinement entry points are declared (include/gaussctrl_refine.h), exported and bound with matching argument counts; the config switch and the new
splatfacto fields exist with their defaults; the schedule predicates of gaussctrl_amd/refine.py against hand-written cases."""
import types

import _abi_header as A

NEW = ("gc_refine_accumulate_views", "gc_refine_plan_workspace_bytes", "gc_refine_plan", "gc_refine_apply", "gc_refine_reset_opacity")


def test_refine_symbols_declared_listed_and_exported():
    import ctypes
    from gaussctrl_amd import _lib
    declared = set(A.names("gaussctrl_refine.h"))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name


def test_refine_bindings_pass_the_declared_number_of_arguments():
    """every call("gc_refine_*", ...) of the host layer passes, with the stream call() appends, as many arguments as the header's prototype
    has parameters; the binding table has that arity too (_abi_header.sites)"""
    declared = A.arities("gaussctrl_refine.h")
    assert declared == {"gc_refine_accumulate_views": 9, "gc_refine_plan_workspace_bytes": 1, "gc_refine_plan": 24, "gc_refine_apply": 16,
                        "gc_refine_reset_opacity": 6}
    sites = A.sites("gaussctrl_amd/refine.py", "gaussctrl_refine.h")
    for name, passed in sites.items():
        assert all(n == declared[name] for n in passed), (name, passed)
    assert set(sites) == set(NEW)


def test_refine_config_switch_and_defaults():
    from gaussctrl_amd.gc_model import GaussCtrlModelConfig
    c = GaussCtrlModelConfig()
    assert c.refine_on_device is False
    want = dict(warmup_length=500, densify_grad_thresh=0.0002, densify_size_thresh=0.01, n_split_samples=2, cull_screen_size=0.15,
                split_screen_size=0.05, stop_screen_size_at=4000)
    assert {k: getattr(c, k) for k in want} == want
    assert all(type(getattr(c, k)) is type(v) for k, v in want.items())
    from gaussctrl_amd.gc_trainer import RefineCallback     # noqa: F401  (exists; the GPU suite runs it)


def test_refine_schedule_hand_cases():
    """R = 100, A = 30, I = 3000, warm-up 500, stop_split_at 15000, stop_screen_size_at 4000 (the defaults)"""
    from gaussctrl_amd.gc_model import GaussCtrlModelConfig
    from gaussctrl_amd.refine import schedule
    c = GaussCtrlModelConfig()
    f = lambda s, n=50: schedule(c, s, n)
    key = lambda r: (r.refine, r.densify, r.cull_only, r.reset)
    assert key(f(500)) == (False, False, False, False)                   # s > warmup_length is strict
    assert key(f(600)) == (True, True, False, False)                     # 600 % 3000 = 600 > 50 + 100
    assert (f(600).cull_by_scale, f(600).by_screen) == (False, True)     # 600 <= I: alpha cull only; 600 < 4000: the screen-size split test
    assert key(f(3100)) == (True, False, False, True)                    # 3100 % 3000 = 100 = R: reset, and 100 > 150 is false
    assert key(f(3000 + 50 + 101)) == (False, False, False, False)       # 3151 is no multiple of R
    assert key(f(3000 + 99 + 101, 99)) == (True, True, False, False)     # 3200 % 3000 = 200 > 99 + 100
    assert key(f(3200, 100)) == (True, False, False, False)              # 200 > 100 + 100 is false: a refinement step that does nothing
    assert (f(3200, 99).cull_by_scale, f(3200, 99).by_screen) == (True, True)
    assert key(f(15000)) == (True, False, True, False)                   # s >= stop_split_at: cull only
    assert key(f(30100)) == (True, False, True, False) and f(30100).cull_by_scale and not f(30100).by_screen
    assert key(f(14900)) == (True, True, False, False) and not f(14900).by_screen
    assert key(f(650)) == (False, False, False, False)
    c2 = GaussCtrlModelConfig(continue_cull_post_densification=False)
    assert key(schedule(c2, 15000, 50)) == (True, False, False, False)
    # a shrunk schedule, as the GPU callback test uses it
    c3 = types.SimpleNamespace(refine_every=5, reset_alpha_every=3, warmup_length=4, stop_split_at=30, stop_screen_size_at=25,
                               continue_cull_post_densification=True)
    got = {s: key(schedule(c3, s, 2)) for s in range(0, 45, 5)}
    assert got == {0: (False, False, False, False), 5: (True, False, False, True), 10: (True, True, False, False), 15: (True, False, False, False),
                   20: (True, False, False, True), 25: (True, True, False, False), 30: (True, False, True, False), 35: (True, False, True, False),
                   40: (True, False, True, False)}
