import asyncio
import os
import shutil
import sys
import tempfile
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))

GOLDEN = REPO / "tests" / "golden"
# the reference project's captured sysfs / debugfs trees (its testdata/ directory: ~7000 small
# kfd topology files), stored as one archive and unpacked once per session
REF_TESTDATA_ARCHIVE = GOLDEN / "reference" / "testdata.tar.xz"


def _short_temp_root() -> str:
    """A writable temporary directory with a short path. The suite binds Unix
    sockets a few directories below its temporary directories (tmp_path, and
    the scratch directories of bench.py and the daemons it starts) and
    sun_path holds 107 bytes: with a long $TMPDIR those binds fail ("AF_UNIX
    path too long")."""
    own = tempfile.gettempdir()
    if len(own) <= 12:
        return own
    for cand in ("/tmp", "/var/tmp", "/dev/shm"):
        if os.path.isdir(cand) and os.access(cand, os.W_OK | os.X_OK):
            return cand
    return own


_TEMP_ROOT = _short_temp_root()
if _TEMP_ROOT != tempfile.gettempdir():
    # only with a long $TMPDIR: the programs the tests start (bench.py, the daemons) inherit it too
    os.environ["TMPDIR"] = _TEMP_ROOT
    tempfile.tempdir = None

# Hypothesis: the suite's verdict must not depend on the draw. "ci" (the
# default) derandomizes and ignores the local example database, so every run
# of the suite tries the same examples; "explore" (HYPOTHESIS_PROFILE=explore)
# draws fresh ones, many more of them (tools/yaml_differential.py records such
# a run). A failure found while exploring goes into the parametrised cases.
try:
    from hypothesis import HealthCheck, settings as _hyp_settings

    _hyp_settings.register_profile("ci", derandomize=True, database=None, max_examples=300, deadline=None,
                                   print_blob=True, suppress_health_check=[HealthCheck.too_slow])
    _hyp_settings.register_profile("explore", derandomize=False, max_examples=int(os.environ.get(
        "MI355X_HYPOTHESIS_EXAMPLES", "10000")), deadline=None, print_blob=True,
        suppress_health_check=[HealthCheck.too_slow])
    _hyp_settings.load_profile(os.environ.get("HYPOTHESIS_PROFILE", "ci"))
except ImportError:  # hypothesis is optional for the non-property tests
    pass


_SHORT_BASETEMP = pytest.StashKey[str]()


@pytest.hookimpl(tryfirst=True)
def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run via gpurun)")
    config.addinivalue_line("markers", "slow: takes more than a few seconds")
    # pytest's base directory is <tmp>/pytest-of-<user>/pytest-<n>; where that is long (a long
    # user name), tmp_path's sockets pass sun_path too: then, and only without --basetemp, a
    # short base directory, removed after a run that passed (a failed run's directories stay)
    if config.option.basetemp is None:
        import getpass
        try:
            user = getpass.getuser()
        except Exception:  # noqa: BLE001 - no passwd entry
            user = "unknown"
        if len(os.path.join(tempfile.gettempdir(), f"pytest-of-{user}", "pytest-000")) > 40:
            config.option.basetemp = tempfile.mkdtemp(prefix="mi355x-pytest-", dir=_TEMP_ROOT)
            config.stash[_SHORT_BASETEMP] = config.option.basetemp


def pytest_sessionfinish(session, exitstatus):
    base = session.config.stash.get(_SHORT_BASETEMP, None)
    if base and exitstatus == 0:
        shutil.rmtree(base, ignore_errors=True)


@pytest.fixture(scope="session", autouse=True)
def _native_built():
    """Build the native core once per session (no-op when up to date)."""
    from rocm_k8s_device_plugin_amd import _build
    _build.ensure_built(hip=None)
    yield


@pytest.fixture(scope="session")
def ref_testdata(tmp_path_factory):
    """The reference's testdata/ directory, unpacked once for the session."""
    import tarfile
    dest = tmp_path_factory.mktemp("reference")
    with tarfile.open(REF_TESTDATA_ARCHIVE) as tar:
        for m in tar.getmembers():   # plain files and directories under testdata/ only
            assert (m.isfile() or m.isdir()) and m.name.split("/")[0] == "testdata" and ".." not in m.name, m.name
            m.mode = 0o755 if m.isdir() else 0o644   # copies of a tree (wrap_kfd_topology) stay writable
        tar.extractall(dest)
    return dest / "testdata"


@pytest.fixture
def mi355x_node(tmp_path):
    from rocm_k8s_device_plugin_amd.testing.fixtures import make_mi355x_node
    return make_mi355x_node(tmp_path / "node")


def run(coro, timeout=60):
    return asyncio.run(asyncio.wait_for(coro, timeout))


@pytest.fixture
def arun():
    return run


def has_gpu() -> bool:
    return os.path.exists("/dev/kfd")
