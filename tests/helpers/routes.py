"""Route observers: prove WHICH path ran, not only that the result is right.

Most GPU tests compare a result with another path that returns the same result, so a dispatch gate can send the work to
a fallback and the suite stays green.  Two observers close that:

* ``count_calls(monkeypatch, owner, name)`` wraps a callable (a Python function on a module / class, or an op of
  ``torch.ops.tmx``) and returns a list that grows by one ``(args, kwargs)`` entry per call.
* ``kernels_run(fn)`` returns the names of the device kernels one call of ``fn`` launched (``torch.profiler``).

Many native gates read their environment knob once per process, so tests reach the "not taken" arm of a gate by shape,
dtype or alignment, never by setting a variable inside the test.
"""
from typing import Any, Callable, Iterable, List, Optional, Tuple

import torch


def count_calls(monkeypatch: Any, owner: Any, name: str, guard: Optional[Callable[..., None]] = None) -> List[Tuple[tuple, dict]]:
    """Replace ``owner.name`` by a forwarding wrapper (undone by ``monkeypatch``); returns the list of recorded calls.

    ``guard(*args, **kwargs)``, when given, runs before the call is forwarded and may raise ``AssertionError`` to keep
    the real callable from running at all.  Ops of ``torch.ops.tmx`` materialise on first access, so ``owner.name`` is
    read once here; the namespace then holds a plain attribute that ``monkeypatch.setattr`` can replace and restore.
    A function patched on a class receives ``self`` as its first recorded argument."""
    orig = getattr(owner, name)
    calls: List[Tuple[tuple, dict]] = []

    def spy(*args: Any, **kwargs: Any) -> Any:
        calls.append((args, kwargs))
        if guard is not None:
            guard(*args, **kwargs)
        return orig(*args, **kwargs)

    spy.__name__ = getattr(orig, "__name__", name)
    spy.__wrapped__ = orig  # type: ignore[attr-defined]
    monkeypatch.setattr(owner, name, spy)
    return calls


def kernels_run(fn: Callable[[], Any]) -> List[str]:
    """Names of the device kernels launched by one ``fn()``, in profiler order.

    One warm-up call runs outside the profile (lazy module loads, allocator growth, first-call plans), then one call
    under the profiler.  A profile without any device event raises: every caller profiles a call that launches at least
    one kernel, so an empty list means the profiler delivered nothing, and a route assertion on it would be vacuous."""
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type.name == "CUDA"]
    if not names:
        raise RuntimeError("the profiler returned no device event for a call that launches kernels")
    return names


def assert_route(names: Iterable[str], present: Iterable[str] = (), absent: Iterable[str] = ()) -> None:
    """Every substring of ``present`` occurs in some kernel name, none of ``absent`` in any."""
    names = list(names)
    for want in present:
        assert any(want in n for n in names), f"kernel {want!r} did not run; ran: {sorted(set(names))}"
    for bad in absent:
        hit = [n for n in names if bad in n]
        assert not hit, f"kernel {bad!r} ran ({hit[0]}); ran: {sorted(set(names))}"
