"""CPU (no GPU needed): the launch plans the engine compiles -- every integer, double and pointer identity of every op -- equal
tests/golden/launch_plans.txt.gz (tests/golden/make_launch_plan_golden.py: format, configurations, how pointers are named)."""
import os

import pytest

import make_launch_plan_golden as G

CONFIGS = G.configs()


@pytest.fixture(scope="module")
def fixture():
    return G.read_fixture()


def test_fixture_lists_exactly_the_configurations(fixture):
    assert list(fixture) == [name for name, _, _ in CONFIGS]
    assert sorted(n for n, (_, _, lines) in fixture.items() if lines) == sorted(n for n, full, _ in CONFIGS if full)
    for name, (ops, sha, lines) in fixture.items():
        if lines:
            assert (G.count_ops(lines), G.digest(lines)) == (ops, sha), name
    assert os.path.getsize(G.FIXTURE) < 1 << 20


@pytest.mark.parametrize("name,full,cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_launch_plan(name, full, cfg, fixture, tmp_path):
    ops, sha, want = fixture[name]
    lines = G.dump_config(cfg)
    if G.digest(lines) == sha and G.count_ops(lines) == ops:
        return
    path = tmp_path / (name + ".txt")
    path.write_text("\n".join(lines) + "\n")
    first = ""
    if want:
        k = next((k for k, (a, b) in enumerate(zip(lines, want)) if a != b), min(len(lines), len(want)))
        first = "; first difference at line %d:\n  got  %s\n  want %s" % (
            k + 1, lines[k] if k < len(lines) else "<end>", want[k] if k < len(want) else "<end>")
    pytest.fail("launch plan %s changed (%d ops, fixture %d): full dump written to %s -- diff it against `python "
                "tests/golden/make_launch_plan_golden.py --dump DIR` of the parent commit%s" % (name, G.count_ops(lines), ops, path, first))
