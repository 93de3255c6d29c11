"""Prepare a checkpoint for release: the reference's
tools/model_converters/publish_model.py.

    python tools/publish_model.py IN.pth OUT.pth

Drops the ``optimizer`` state, saves, and renames the file to
``OUT-{first 8 hex digits of its sha256}.pth``.
"""
import argparse
import hashlib
import os
import os.path as osp
import sys

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Process a checkpoint to be '
                                'published')
    p.add_argument('in_file', help='input checkpoint filename')
    p.add_argument('out_file', help='output checkpoint filename')
    return p.parse_args(argv)


def process_checkpoint(in_file, out_file):
    import torch
    ckpt = torch.load(in_file, map_location='cpu')
    ckpt.pop('optimizer', None)  # sensitive and large
    torch.save(ckpt, out_file)
    h = hashlib.sha256()
    with open(out_file, 'rb') as f:
        for block in iter(lambda: f.read(1 << 20), b''):
            h.update(block)
    stem = out_file[:-len('.pth')] if out_file.endswith('.pth') else out_file
    final = f'{stem}-{h.hexdigest()[:8]}.pth'
    os.replace(out_file, final)
    return final


def main(argv=None):
    args = parse_args(argv)
    print(process_checkpoint(args.in_file, args.out_file))


if __name__ == '__main__':
    main()
