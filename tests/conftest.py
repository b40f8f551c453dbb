import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


# Lines the tests want in the run's terminal summary -- it is printed under -q as well, so the driver's log tail says which
# sizes ran ("10M x 768 / 50M x 128 FULL SIZE") and which id-equality fractions were measured.
SUMMARY_LINES = []


def pytest_terminal_summary(terminalreporter, exitstatus, config):
    if SUMMARY_LINES:
        terminalreporter.write_sep("-", "flatnav_amd: sizes and measured parity fractions")
        for line in SUMMARY_LINES:
            terminalreporter.write_line(line)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    config.addinivalue_line("markers", "slow: long-running CPU test")


# Result-pinning tests first, anything that measures time or drives many host threads last: under `-x` a late
# failure can then never hide the parity suites.  Files not named keep their alphabetical place in the middle.
_ORDER = ["test_golden", "test_gpu_parity", "test_gpu_round5", "test_gpu_round6", "test_gpu_configs", "test_cpp_api",
          "test_gpu_python_api", "test_gpu_round4", "test_gpu_round3", "test_gpu_device_build", "test_gpu_fullsize",
          "test_gpu_bench", "test_gpu_multi_device"]


def pytest_collection_modifyitems(session, config, items):
    def rank(item):
        name = os.path.splitext(os.path.basename(str(item.fspath)))[0]
        if name in _ORDER:
            return _ORDER.index(name) + (0 if _ORDER.index(name) < 5 else 1000)
        return 500

    items.sort(key=rank)  # stable: the order inside a file is kept


@pytest.fixture(scope="session")
def oracle_mod():
    from oracle import oracle as orc

    orc.build()
    return orc


class ReferenceAnswers:
    """The reference's answers on the tests' own inputs, stored in tests/golden/reference/answers.npz, so that the tests that
    pin the product against the executed reference run where the reference sources are absent (a clean checkout, the GPU
    box).  `answers(key, compute)`: where oracle/_ref was built, compute(ref) runs live and must equal the stored answer bit
    for bit; elsewhere the stored answer is returned.  FLATNAV_RECORD_REFERENCE=1 (with oracle/_ref built) rewrites them."""

    PATH = os.path.join(ROOT, "tests", "golden", "reference", "answers.npz")

    def __init__(self, live):
        import numpy as np

        self.np, self.live = np, live
        self.record = live is not None and os.environ.get("FLATNAV_RECORD_REFERENCE") == "1"
        self.stored = dict(np.load(self.PATH)) if os.path.exists(self.PATH) else {}

    def __call__(self, key, compute):
        np = self.np
        if self.live is None:
            assert key in self.stored, "no stored reference answer for %s" % key
            return self.stored[key]
        got = np.asarray(compute(self.live))
        if self.record:
            self.stored[key] = got
        else:
            want = self.stored.get(key)
            assert want is not None, "no stored reference answer for %s (record: FLATNAV_RECORD_REFERENCE=1)" % key
            assert want.dtype == got.dtype and want.shape == got.shape and want.tobytes() == got.tobytes(), key
        return got

    def save(self):
        if self.record:
            self.np.savez_compressed(self.PATH, **dict(sorted(self.stored.items())))


@pytest.fixture(scope="session")
def ref_answers(oracle_mod):
    A = ReferenceAnswers(oracle_mod.ref_lib())
    yield A
    A.save()
