"""A file worker for plan pages: the consumer side of the reference's file queue, in-process and standard-library only.

The reference's agent starts a process that takes ``(kind, path, payload)`` tuples off a queue and writes them with
OpenCV and imageio (``visual_mpc/agent/utils/file_saver.py:23-53``); the controllers only ever call ``put`` on what they
are handed as ``verbose_worker``.  ``PlanPageWriter`` offers that ``put`` and writes at once:

    ('path', directory)                 everything after it is written below ``directory`` (created when missing)
    ('txt_file', path, text)            ``text`` and a newline
    ('img', path, uint8 [H, W, 3])      an RGB PNG (``utils/png.py``)
    ('mov', path, uint8 [T, H, W, 3])   an animated PNG, 4 frames per second unless a fourth element gives the rate
    None                                end of stream (nothing to do here)

It writes PNG where the reference writes JPEG and GIF (lossless, zlib only) and says so through ``asset_extensions``,
which ``build_plan_messages`` reads to name the files - so the page points at what is on the disk.
"""
import os

from visual_foresight_amd.utils.png import write_apng, write_png


class PlanPageWriter(object):
    asset_extensions = ('png', 'png')       # (movies, images)

    def __init__(self, root='.'):
        self.root = root
        self.written = []       # the paths written so far

    def _open_path(self, rel):
        path = os.path.join(self.root, rel)
        parent = os.path.dirname(path)
        if parent and not os.path.isdir(parent):
            os.makedirs(parent)
        return path

    def put(self, message):
        if message is None:
            return
        kind = message[0]
        if kind == 'path':
            self.root = message[1]
            if not os.path.isdir(self.root):
                os.makedirs(self.root)
            return
        if kind not in ('txt_file', 'img', 'mov'):
            raise ValueError('unknown file message %r' % (kind,))
        path = self._open_path(message[1])
        if kind == 'txt_file':
            with open(path, 'w') as f:
                f.write(message[2])
                f.write('\n')
        elif kind == 'img':
            write_png(path, message[2])
        else:
            write_apng(path, message[2], fps=message[3] if len(message) == 4 else 4)
        self.written.append(path)
