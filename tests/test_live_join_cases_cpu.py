"""CPU: the cases of tests/live_join_cases.py. The restated arithmetic of the
backward's join (prefix by thread, wave and workgroup; chunk dealing; the
search for a list position's ray) gives the plain concatenation of the per-ray
lists, every chunk below the count is stored by exactly one workgroup, and
each case hits the condition it is named for."""
import numpy as np
import pytest

import live_join_cases as jc

NAMES = [c.name for c in jc.cases()]


def _regime(c, d):
    total = int(d["counts"].sum())
    lim = jc.light_limit(c.M, c.rows_max, c.stash_rows)
    return total, lim, (lim > 0 and total <= lim)


@pytest.mark.parametrize("name", NAMES)
def test_join_equals_concatenation(name):
    c, d = jc.case(name), jc.build(name)
    total, lim, light = _regime(c, d)
    assert len(d["rows"]) == total <= c.M
    assert d["live"].sum() == total and np.array_equal(np.flatnonzero(d["live"]), np.sort(d["rows"]))
    out, t, owners = jc.join(d, c.M, c.G, lim)
    assert t == total
    assert np.array_equal(out[:total], d["rows"])
    assert (out[total:] == -1).all()                      # nothing is stored past the total
    nch = -(-total // jc.CHUNK)
    assert sorted(owners) == list(range(nch))             # every chunk below the count ...
    assert all(len(v) == 1 for v in owners.values())      # ... by exactly one workgroup
    assert all(v[0] == ch % c.G for ch, v in owners.items())
    # the prefix alone: a ray's absolute position is the concatenation's
    pos, base, _ = jc.join_prefix(d["counts"], c.N)
    absolute = pos + np.repeat(base, 64 * jc.RAYS_PER_THREAD)
    assert np.array_equal(absolute[:c.N], np.cumsum(d["counts"]) - d["counts"])


def test_shapes_the_cases_are_named_for():
    by = {c.name: c for c in jc.cases()}
    assert {by[f"n{n}"].N for n in (1, 15, 16, 17, 63, 64, 65)} == {1, 15, 16, 17, 63, 64, 65}
    assert by["n4096_light"].N == by["n4096_heavy"].N == by["wg5"].N == jc.CAP == 4096
    tot = {n: int(jc.build(n)["counts"].sum()) for n in by}
    reg = {n: _regime(by[n], jc.build(n))[2] for n in by}
    # the bench's shape: 256 workgroups, a live fraction of the allocation under 0.1, the stash route
    assert by["n4096_light"].G == 256 and reg["n4096_light"] and 0.05 < tot["n4096_light"] / by["n4096_light"].M < 0.1
    assert not reg["n4096_heavy"] and 1 < -(-tot["n4096_heavy"] // 32) / by["n4096_heavy"].G <= 2
    assert tot["all_zero"] == 0
    d = jc.build("last_ray_only")
    assert tot["last_ray_only"] == 1 and d["counts"][-1] == 1 and by["last_ray_only"].N == 65
    assert (jc.build("one_each")["counts"] == 1).all() and not reg["one_each"]
    assert (jc.build("one_each_light")["counts"] == 1).all() and reg["one_each_light"]
    d = jc.build("long_ray")
    k = int(np.argmax(d["counts"]))
    first = int(d["counts"][:k].sum())
    assert d["counts"][k] > 64 and first // 32 + 2 <= (first + d["counts"][k] - 1) // 32   # spans chunks
    assert (tot["t31"], tot["t32_on_ray_edge"], tot["t33_on_ray_edge"], tot["t33_in_ray"]) == (31, 32, 33, 33)
    edges = lambda n: set(np.cumsum(jc.build(n)["counts"]).tolist())  # noqa: E731
    assert 32 in edges("t32_on_ray_edge") and 32 in edges("t33_on_ray_edge") and 32 not in edges("t33_in_ray")
    c, d = by["overflow_ray"], jc.build("overflow_ray")
    assert c.counts[-1] > 0 and d["counts"][-1] == 0 and d["rays"][-1, 1] + d["rays"][-1, 2] > c.M > d["rays"][-1, 1]
    g = jc.build("gaps")["counts"]
    assert g[0] > 0 and g[-1] == 0 and ((g[1:-1] == 0) & (g[:-2] > 0)).any() and ((g[1:-1] == 0) & (g[2:] > 0)).any()
    # the switch: the count at dw_rows runs the stash route, one more the slab route
    assert tot["at_dw_rows"] == jc.ROWS_MAX and reg["at_dw_rows"]
    assert tot["past_dw_rows"] == jc.ROWS_MAX + 1 and not reg["past_dw_rows"]
    # 1..5 chunks on a workgroup
    for n in (1, 2, 3, 4, 5):
        c = by[f"wg{n}"]
        per = [len(jc.chunks_of(b, c.G, tot[c.name])) for b in range(c.G)]
        assert max(per) == n and not reg[c.name], (c.name, per)
        assert n < 5 and c.G == 3 or n == 5 and c.G == 256
    assert max(len(jc.chunks_of(b, 256, 262144)) for b in range(256)) == jc.MAX_CHUNKS
    # both routes and every kind of last round are met: 1 or 2 chunks left (half chunks), 3, 0
    left = {len(jc.chunks_of(b, by[n].G, tot[n])) % 4 for n in by for b in range(by[n].G)}
    assert left == {0, 1, 2, 3}
    assert any(reg.values()) and not all(reg.values())


def test_planned_lists_are_the_composites_layout():
    """ray_rows holds ray n's live rows, ascending, from the ray's first row on."""
    for name in ("gaps", "long_ray", "overflow_ray"):
        d = jc.build(name)
        rr = jc.planned_ray_rows(d)
        for n in range(d["N"]):
            o, k = int(d["rays"][n, 1]), int(d["counts"][n])
            got = rr[o:o + k]
            assert (np.diff(got) > 0).all() and d["live"][got].all()
            assert ((got >= o) & (got < o + d["rays"][n, 2])).all()
