import gc
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(autouse=True)
def _collect_cycles_between_tests():
    """A model and its graph-replay helper point at each other (Aggregator._replay.module), so a test's models -- with their captured
    hipGraphs, graph pool and workspaces -- are freed by Python's cyclic GC, at whatever allocation it happens to run on.  Inside a
    later test's stream capture those finalisers are not allowed to run: collect each test's cycles when it ends instead."""
    yield
    gc.collect()


@pytest.fixture(scope="session")
def golden_dir():
    return os.path.join(ROOT, "tests", "golden")
