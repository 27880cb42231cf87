"""bench.py's command line (host side, no device): a plain run measures the headline alone, --full adds the side measurements, the
EM sweeps, the CPU baseline and the live K1 traffic, each of which --no-extra / --no-cpu-baseline / --no-live-pmc can leave out."""
import pytest

import bench

PLAIN = ["--gpus", "1", "--steps", "20", "--warmup", "5"]


def test_a_plain_run_leaves_out_what_the_headline_does_not_need():
    a = bench.parse_args(PLAIN)
    assert not a.full
    assert a.no_cpu_baseline and a.no_extra and a.no_live_pmc
    assert (a.steps, a.warmup, a.gpus) == (20, 5, 1)


def test_a_plain_run_keeps_its_dump():
    a = bench.parse_args(PLAIN + ["--dump-outputs", "out"])
    assert a.dump_outputs == "out" and a.no_extra


def test_full_measures_everything_unless_told_otherwise():
    a = bench.parse_args(PLAIN + ["--full"])
    assert a.full
    assert not (a.no_cpu_baseline or a.no_extra or a.no_live_pmc)


@pytest.mark.parametrize("flag,attr", [("--no-extra", "no_extra"), ("--no-cpu-baseline", "no_cpu_baseline"),
                                       ("--no-live-pmc", "no_live_pmc")])
def test_full_leaves_out_one_part_at_a_time(flag, attr):
    a = bench.parse_args(PLAIN + ["--full", flag])
    assert {k: getattr(a, k) for k in ("no_extra", "no_cpu_baseline", "no_live_pmc")} == \
        {k: k == attr for k in ("no_extra", "no_cpu_baseline", "no_live_pmc")}


def test_only_picks_side_measurements_of_a_full_run(capsys):
    assert bench.parse_args(PLAIN + ["--full", "--only", "cfg2,em"]).only == "cfg2,em"
    with pytest.raises(SystemExit) as e:
        bench.parse_args(PLAIN + ["--only", "cfg2"])
    assert e.value.code == 2
    assert "--full" in capsys.readouterr().err
