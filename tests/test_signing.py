"""tools/sign.sh: detached GPG signatures of native sources."""

import os
import shutil
import subprocess
import tempfile

import pytest

from .helpers import ROOT


@pytest.fixture
def gnupg_home(tmp_path):
    """A private GNUPGHOME with a short path: gpg-agent listens on unix sockets
    inside it (S.gpg-agent.browser is the longest name), and a socket path is
    limited to 107 bytes — pytest's tmp_path under a deep TMPDIR exceeds that
    and the agent then fails to start. The agent is stopped afterwards."""
    longest = len("/S.gpg-agent.browser")
    home = None
    for base in (str(tmp_path), tempfile.gettempdir(), "/tmp", "/var/tmp", "/dev/shm"):
        if os.path.isdir(base) and os.access(base, os.W_OK | os.X_OK) and len(base) + 12 + longest <= 107:
            home = tempfile.mkdtemp(prefix="mpx", dir=base)  # mode 0700
            break
    if home is None:  # no short writable directory: gpg will say what it cannot do
        home = str(tmp_path / "gnupg")
        os.mkdir(home, 0o700)
    try:
        yield home
    finally:
        if shutil.which("gpgconf"):
            subprocess.run(["gpgconf", "--kill", "gpg-agent"], env=dict(os.environ, GNUPGHOME=home),
                           capture_output=True, timeout=60)
        shutil.rmtree(home, ignore_errors=True)


@pytest.mark.skipif(shutil.which("gpg") is None, reason="gpg not installed")
def test_sign_and_verify(tmp_path, gnupg_home):
    env = dict(os.environ, GNUPGHOME=gnupg_home)
    r = subprocess.run(["gpg", "--batch", "--passphrase", "", "--quick-gen-key", "mpx test <mpx@example.invalid>",
                        "ed25519", "sign", "never"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    src = tmp_path / "main.c"
    src.write_text("int main(void) { return 0; }\n")
    sign = os.path.join(ROOT, "tools", "sign.sh")
    r = subprocess.run([sign, str(src)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "main.c.asc").read_text().startswith("-----BEGIN PGP SIGNATURE-----")
    assert subprocess.run([sign, "--verify", str(src)], env=env, capture_output=True, timeout=120).returncode == 0
    src.write_text("int main(void) { return 1; }\n")  # tampered
    assert subprocess.run([sign, "--verify", str(src)], env=env, capture_output=True, timeout=120).returncode != 0
