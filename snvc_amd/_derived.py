"""When a value derived from tensors (packed weights, a folded BatchNorm, a data-gradient layer, ...) is still valid.

A derived value stays valid exactly as long as its sources are the same tensor objects, at the same address, unmodified.  A stamp
holds, per source, the tensor itself (compared with ``is``: tuple equality would fall back to ``Tensor.__eq__``), its
``data_ptr()`` and its ``_version``; holding the tensor means no other tensor can come back at its address while the stamp lives.
``data_ptr()`` is a unified virtual address, so it also tells devices apart.  Every in-place update that goes through an
autograd-visible tensor (``optimizer.step()``, ``load_state_dict``, ``p.copy_()`` under ``no_grad``) bumps ``_version``; the
package's own raw-pointer writes into a caller's buffer bump it too (``ops._written``).  Writes through ``.data``
(``p.data.mul_(2)``) bump nothing: ``submodule.invalidate_plans()`` bumps ``_GENERATION`` after them, which every stamp holds."""

_GENERATION = [0]


def invalidate_all() -> None:
    """Void every stamp of the process."""
    _GENERATION[0] += 1


def stamp(sources, extra=()) -> tuple:
    """The state of ``sources`` (tensors or None) now, with the generation and the site's own ``extra`` key values."""
    return _GENERATION[0], extra, tuple(None if t is None else (t, t.data_ptr(), t._version) for t in sources)


def fresh(st, sources, extra=()) -> bool:
    """Is ``st`` (a stamp or None) still the state of ``sources`` -- the same tensors, unmodified -- and of ``extra``?"""
    if st is None or st[0] != _GENERATION[0] or st[1] != extra or len(st[2]) != len(sources):
        return False
    for s, t in zip(st[2], sources):
        if t is None:
            if s is not None:
                return False
        elif s is None or s[0] is not t or s[1] != t.data_ptr() or s[2] != t._version:
            return False
    return True


def derived(store, name, sources, build, extra=()):
    """``store[name]``'s value while it is fresh for ``sources`` / ``extra``, else ``build()``'s (stored with its stamp)."""
    hit = store.get(name)
    if hit is not None and fresh(hit[0], sources, extra):
        return hit[1]
    st = stamp(sources, extra)
    value = build()
    store[name] = (st, value)
    return value


def tag(t, value) -> tuple:
    """``value`` tagged to the tensor ``t``, valid while t keeps its address and version (``tagged``).  The tag does not hold t:
    it lives in t's own ``__dict__``, and a reference cycle would keep device memory alive until the cyclic collector runs."""
    return value, t.data_ptr(), t._version


def tagged(t, tg):
    """The value of the tag ``tg`` (or None) if ``t`` has not been written to since it was tagged, else None."""
    return tg[0] if tg is not None and tg[1] == t.data_ptr() and tg[2] == t._version else None
