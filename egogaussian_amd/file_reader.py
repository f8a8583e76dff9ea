"""The device file reader: what png.PngReader and jpeg.JpegReader share, which is everything but the format.

    load_files        files (bytes or paths) -> (blobs, names, parsed): the host's share of a read, the parse function given
    upload_layout     where the descriptors, the second table and the files of one batch lie in its one upload
    stage             writes that upload into (pinned) host memory
    DeviceFileReader  file bytes -> device uint8 [h, w, C]: owns the pinned staging, the device buffer the files and their tables are uploaded
                      to, the scratch, the outputs and the status words, the guard bytes around all of them, and the loop over the batches

A format supplies (the hooks below DeviceFileReader.decode): its parse and plan, the second table of its C entry and the count that goes with
it, the size of its scratch and of its status record, and its launch.  Nothing here names a format.
"""
import numpy as np
import torch

from . import lib as _lib
from . import _hip


def _up(v, a):
    return (v + a - 1) // a * a


def load_files(files, parse_one):
    """files: bytes (bytearray, memoryview) or paths -> (blobs, names, parsed): names[i] is "file i" or "file i (path)", parsed[i] =
    parse_one(blobs[i]).  No device work; a ValueError of parse_one is raised again with the file's name in front."""
    blobs, names = [], []
    for i, f in enumerate(files):
        if isinstance(f, (bytes, bytearray, memoryview)):
            blobs.append(f)
            names.append(f"file {i}")
        else:
            with open(f, "rb") as fh:
                blobs.append(fh.read())
            names.append(f"file {i} ({f})")
    parsed = []
    for name, b in zip(names, blobs):
        try:
            parsed.append(parse_one(b))
        except ValueError as e:
            raise ValueError(f"{name}: {e}") from None
    return blobs, names, parsed


def upload_layout(desc, second):
    """One batch's upload: desc at 0, the second table at the next multiple of 256, the files behind the next multiple of 256 (each at its
    file_offset from there).  -> (offset of the second table, offset of the files)."""
    at_second = _up(desc.nbytes, 256)
    return at_second, at_second + _up(second.nbytes, 256)


def stage(host, desc, second, blobs):
    """Writes the upload of upload_layout into `host` (numpy uint8); the bytes between the pieces are left as they are."""
    at_second, at_files = upload_layout(desc, second)
    host[:desc.nbytes] = desc.view(np.uint8).reshape(-1)
    host[at_second:at_second + second.nbytes] = second.view(np.uint8).reshape(-1)
    for d, b in zip(desc, blobs):
        at = at_files + int(d["file_offset"])
        host[at:at + len(b)] = np.frombuffer(b, dtype=np.uint8)


class DeviceFileReader:
    """Files -> device uint8 [h, w, C] tensors.  Owns the pinned staging, the device buffer the files and their tables are uploaded to, the
    scratch, the outputs and the status words; each grows to what the largest batch so far needed and never shrinks (max_file_bytes /
    max_pixels reserve it up front).  Per batch of at most `batch` files: the host walks the file's structure (load), ONE upload, the
    format's launches, ONE read of the status words.  A file the device refuses leaves the other files of its call decoded (last_results)
    and its own slot untouched.  guard > 0 (a multiple of 256) is for tests: every byte of the device buffers that a call is not entitled to
    -- `guard` bytes before and behind each buffer, the gaps between the output slots, and everything behind the status words, the scratch
    bytes and the outputs IN USE up to the end of their allocations -- holds GUARD_BYTE before the launches, and check_guards() says
    whether all of it still does."""
    GUARD_BYTE = 0xA5

    def __init__(self, device, batch=32, max_file_bytes=0, max_pixels=0, guard=0):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"{self.NAME}: the {self.FORMAT} decoder has no CPU path (device {self.device}); {self.HOST_READER} is the host reader")
        self.batch, self.guard = int(batch), int(guard)
        if self.batch < 1 or self.batch > 65535 or self.guard < 0 or self.guard % 256:
            raise ValueError(f"{self.NAME}: batch of 1 .. 65535, guard a multiple of 256")
        self._dev, self._pin = {}, None
        self.host_reads = 0                                             # reads of the status words (one per batch)
        self.last_status, self.last_results = [], []                    # of the last read(): a refused batch leaves them to look at
        self._slack_ok, self._gaps = True, []
        if max_file_bytes or max_pixels:
            up = self.batch * (_up(int(max_file_bytes), 16) + 4096)
            self._pinned(up)
            self._buffer("blob", up)
            self._buffer("out", self.batch * _up(3 * int(max_pixels) + self.guard, 256))
            self._buffer("scratch", self._reserve_scratch(int(max_file_bytes), int(max_pixels)))

    def _pinned(self, nbytes):
        if self._pin is None or self._pin.numel() < nbytes:
            self._pin = torch.empty(_up(nbytes, 4096), dtype=torch.uint8).pin_memory()
        return self._pin

    def _buffer(self, name, nbytes):
        """The inner `nbytes` (at least) of a device buffer with `guard` bytes on either side."""
        g, t = self.guard, self._dev.get(name)
        if t is None or t.numel() < nbytes + 2 * g:
            t = torch.full((_up(nbytes, 4096) + 2 * g,), self.GUARD_BYTE, dtype=torch.uint8, device=self.device)
            self._dev[name] = t
        return t[g:t.numel() - g]

    def _intact(self, t):
        return bool((t == self.GUARD_BYTE).all())

    def check_guards(self):
        """True when every guard byte still holds GUARD_BYTE: around the buffers, between and behind the output slots of the last read(),
        and -- looked at after every batch of that read() -- behind the status words and the scratch bytes the batch used."""
        g = self.guard
        ok = self._slack_ok
        for name, t in self._dev.items():
            if g:
                ok = ok and self._intact(t[:g]) and self._intact(t[t.numel() - g:])
        for lo, hi in self._gaps:
            ok = ok and self._intact(self._dev["out"][lo:hi])
        return ok

    def read(self, files):
        """files: a list of bytes or paths -> a list of device uint8 [h, w, C] tensors, views into the reader's output buffer, valid until the
        next call.  ValueError for a file the format's parse() refuses, and for a file the device refuses: it names the file's index (and
        path) and says what the status word says; the other files of the call are decoded all the same (last_results)."""
        return self.decode(*self.load(files))

    @classmethod
    def load(cls, files):
        """The host's share of read(): files (bytes or paths) -> (blobs, names, parsed), parsed[i] = _parse_one(blob).  No device work;
        ValueError for a file parse() refuses."""
        return load_files(files, cls._parse_one)

    def decode(self, blobs, names, parsed):
        """The device's share of read(), from what load() returned."""
        self._slack_ok, self._gaps = True, []
        if not parsed:
            return []
        whole = self._plan(parsed, self.guard)
        out = self._buffer("out", whole["out_bytes"])
        g0 = self.guard
        if g0:
            out.fill_(self.GUARD_BYTE)
            self._gaps.append((g0 + whole["out_bytes"], g0 + out.numel()))      # behind the last slot, up to the end of the allocation
        results, failures = [], []
        lib = _lib.load()
        for lo in range(0, len(parsed), self.batch):
            part = parsed[lo:lo + self.batch]
            p = self._plan(part, g0)
            n = len(part)
            second, count = self._second_table(p)
            at_second, at_files = upload_layout(p["desc"], second)
            up_bytes = at_files + p["files_bytes"]
            pin = self._pinned(up_bytes)
            stage(pin.numpy(), p["desc"], second, blobs[lo:lo + n])
            blob = self._buffer("blob", up_bytes)
            blob[:up_bytes].copy_(pin[:up_bytes], non_blocking=True)
            need = self._scratch_need(lib, n, p)
            scratch = self._buffer("scratch", need)
            status = self._buffer("status", self._status_allocation())
            used = self._status_bytes(n)
            base = int(whole["desc"]["out_offset"][lo])                  # this batch's slots inside the call's output buffer
            self.last_call = (n, blob.data_ptr() + at_files, p["files_bytes"], pin.data_ptr(), blob.data_ptr(), pin.data_ptr() + at_second,
                              blob.data_ptr() + at_second, count, out.data_ptr() + base, p["out_bytes"], status.data_ptr(), scratch.data_ptr(), need)
            if g0:                                                      # everything behind the bytes in use holds the guard byte
                status[used:].fill_(self.GUARD_BYTE)
                scratch[need:].fill_(self.GUARD_BYTE)
            with _hip.device_ctx(self.device):
                self._launch(lib, self.last_call, n, status)
            words = status[:used].view(torch.int32).cpu().tolist()      # (synchronises: the staging may be refilled)
            self.host_reads += 1
            if g0:
                self._slack_ok = self._slack_ok and self._intact(status[used:]) and self._intact(scratch[need:])
            words = [w & 0xFFFFFFFF for w in self._after_words(words, lo, n)]
            for k, (d, w) in enumerate(zip(p["desc"], words)):
                W, H, C = int(d["width"]), int(d["height"]), int(d["channels"])
                o = base + int(d["out_offset"])
                results.append(out[o:o + H * W * C].view(H, W, C))
                if g0:
                    self._gaps.append((g0 + o + H * W * C, g0 + o + _up(H * W * C + g0, 256)))
                if w:
                    failures.append(f"{names[lo + k]}: {self.status_text(w)} (status {w})")
            self.last_status = (self.last_status if lo else []) + words
        self.last_results = results
        if failures:
            raise ValueError(f"{self.NAME}.read: " + "; ".join(failures))
        return results

    # ---- what a format supplies: NAME, FORMAT and HOST_READER for the messages, status_text, and ---------------------------------------------
    # _parse_one(blob)             static: the format's parse() with the file's length, an entry of `parsed`
    # _shape(entry)                static: (W, H, C) of such an entry
    # _plan(part, gap)             the descriptor tables and totals of a batch: dict with desc (fields width, height, channels, file_offset,
    #                              out_offset), files_bytes, out_bytes and whatever the hooks below read
    # _second_table(p)             -> (the array uploaded behind desc, the count the C entry takes with it)
    # _scratch_need(lib, n, p)     the scratch bytes of a batch
    # _reserve_scratch(max_file_bytes, max_pixels)     the scratch bytes to reserve up front
    # _status_allocation()         the size of the status buffer
    # _launch(lib, call, n, status)     the launches: call is last_call, the thirteen leading arguments of the C entry
    def _status_bytes(self, n):
        """The bytes a batch of n files reads back in its one read: a status word per file, first."""
        return 4 * n

    def _after_words(self, words, lo, n):
        """words: the int32 words of that read, for the batch that begins at file `lo` -> its n status words."""
        return words
