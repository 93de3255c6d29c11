"""COCO error analysis (C75 / C50 / Loc / Sim / Oth / BG / FN per category)
of a bbox results json, on the device: the reference's
tools/analysis_tools/coco_error_analysis.py, same arguments.

    python tools/coco_error_analysis.py result.json out_dir \
        [--ann data/coco/annotations/instances_val2017.json] [--types bbox]

Writes out_dir/bbox/aps.json and, when matplotlib imports, the reference's
figures out_dir/bbox/bbox-{class}-{area}.png; prints the all-class table.
"""
import os
import sys
from argparse import ArgumentParser

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    parser = ArgumentParser(description='COCO Error Analysis Tool')
    parser.add_argument('result', help='result file (json format) path')
    parser.add_argument('out_dir', help='dir to save analyze result images')
    parser.add_argument(
        '--ann',
        default='data/coco/annotations/instances_val2017.json',
        help='annotation file path')
    parser.add_argument(
        '--types', type=str, nargs='+', default=['bbox'], help='result types')
    args = parser.parse_args()
    from ld_amd.coco_analysis import TYPES, coco_error_analysis
    out = coco_error_analysis(args.result, args.ann, out_dir=args.out_dir,
                              types=args.types)
    print('area     ' + ' '.join(f'{t:>6}' for t in TYPES))
    for area, row in out['aps']['allclass'].items():
        print(f'{area:<8} ' + ' '.join(f'{row[t]:6.3f}' for t in TYPES))


if __name__ == '__main__':
    main()
