"""mmseq -contrasts FILE without a device: the contrasts file is read against the header's ids before the reads and before any device
work, so each malformed file ends the run with exit code 1 and its own message (file, line, cause)."""
import pytest

from oracle import host_oracle as H
from test_cli import dataset, run


@pytest.fixture(scope="module")
def hits(tmp_path_factory):
    d = tmp_path_factory.mktemp("contrast_cli")
    p = d / "x.hits"
    p.write_bytes(H.write_hits_text(dataset(n_reads=300)))
    return d, p


BAD = [
    ("a\tT0000001\tT0000002\nb\tT0000003\tNOPE\n", 2, "unknown transcript id 'NOPE' in the denominator"),
    ("# allele pairs\n\na\t\tT0000002\n", 3, "empty numerator"),
    ("a\tT0000001\t\n", 1, "empty denominator"),
    ("a\tT0000001,T0000002,T0000001\tT0000003\n", 1, "transcript 'T0000001' twice in the numerator"),
    ("a\tT0000001\tT0000002\na\tT0000003\tT0000004\n", 2, "duplicate contrast name 'a'"),
    ("a\tT0000001\n", 1, "expected 3 tab-separated fields"),
    ("a\tT0000001\tT0000002\textra\n", 1, "expected 3 tab-separated fields"),
    ("a T0000001 T0000002\n", 1, "expected 3 tab-separated fields"),
]


@pytest.mark.parametrize("text,line,cause", BAD)
def test_a_malformed_contrasts_file_exits_1_before_any_device_work(hits, text, line, cause):
    d, p = hits
    f = d / "bad.contrasts"
    f.write_text(text)
    r = run(["-contrasts", str(f), str(p), str(d / "out")], timeout=60)
    err = r.stderr.decode()
    assert r.returncode == 1 and ("Error: %s:%d: %s" % (f, line, cause)) in err, err
    assert "no HIP device available" not in err
    assert not (d / "out.k").exists()                    # nothing was read or written yet


def test_a_missing_or_empty_contrasts_file(hits):
    d, p = hits
    r = run(["-contrasts", str(d / "nope"), str(p), str(d / "out")], timeout=60)
    assert r.returncode == 1 and b"Error: cannot open contrasts file" in r.stderr
    (d / "none.contrasts").write_text("# nothing\n\n")
    r = run(["-contrasts", str(d / "none.contrasts"), str(p), str(d / "out")], timeout=60)
    assert r.returncode == 1 and b"no contrasts" in r.stderr and b"no HIP device available" not in r.stderr


def test_contrasts_on_several_devices_are_refused(hits):
    d, p = hits
    f = d / "ok.contrasts"
    f.write_text("a\tT0000001\tT0000002\n")
    r = run(["-gpus", "2", "-contrasts", str(f), str(p), str(d / "out")], timeout=60)
    assert r.returncode == 1 and b"Error: -contrasts reads the chain's trace on one device: it cannot be combined with -gpus > 1." in r.stderr
    assert b"no HIP device available" not in r.stderr


def test_the_usage_text_names_the_flag():
    r = run(["-help"])
    assert r.returncode == 1 and b"  -contrasts FILE " in r.stderr and b".contrasts.mmseq" in r.stderr
