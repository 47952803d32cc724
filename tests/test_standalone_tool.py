"""tools/standalone_validate.hip calls the launchers directly, outside the
extension build, so nothing else notices when a launcher signature leaves
it behind. A syntax-only pass over the translation unit (about 2 s, no GPU)
keeps it compiling."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hipcc():
    found = shutil.which('hipcc')
    if found:
        return found
    rocm = '/opt/rocm/bin/hipcc'
    return rocm if os.access(rocm, os.X_OK) else None


def test_standalone_validate_compiles():
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip('hipcc is not on the path or under /opt/rocm/bin')
    res = subprocess.run(
        [hipcc, '--offload-arch=gfx950', '-std=c++17', '-fsyntax-only',
         os.path.join('tools', 'standalone_validate.hip')],
        cwd=ROOT, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
