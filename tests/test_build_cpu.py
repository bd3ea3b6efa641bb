"""iodine_amd.build without a GPU: the source list matches csrc/ on disk, every header is a dependency of the objects, and the
source digest follows the headers' bytes."""
import glob
import os
import shutil

from iodine_amd import build


def _names(pattern):
    return {os.path.basename(p) for p in glob.glob(os.path.join(build.CSRC, pattern))}


def test_sources_are_the_hip_and_cpp_files_on_disk():
    assert len(build.SOURCES) == len(set(build.SOURCES))
    assert set(build.SOURCES) == _names('*.hip') | _names('*.cpp')


def test_every_header_is_a_dependency():
    headers = {os.path.abspath(h) for h in build.HEADERS}
    for name in _names('*.h'):
        assert os.path.join(build.CSRC, name) in headers
    assert os.path.join(build.ROOT, 'include', 'iodine_hip.h') in headers


def test_source_digest_follows_every_header(tmp_path, monkeypatch):
    csrc = tmp_path / 'csrc'
    shutil.copytree(build.CSRC, csrc, ignore=shutil.ignore_patterns('build'))
    real = build.source_digest()
    monkeypatch.setattr(build, 'CSRC', str(csrc))
    assert build.source_digest() == real                               # the copy digests like the tree
    for name in sorted(_names('*.h')):
        before = build.source_digest()
        with open(csrc / name, 'ab') as f:
            f.write(b'\n')
        assert build.source_digest() != before, name
