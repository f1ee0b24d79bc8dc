"""The piece plans of the batch calls (csrc/gpsiq_pieces.h) on the CPU: tests/piece_plans.cpp prints them for 2.6, 10 and 25 Msps,
12 and 16 channels, both sides of ref_kernel_bound, block counts either side of every branch, and GPSIQ_PIECE_BLOCKS unset and at
0 1 2 3 5 8 40 -1.  The tables below are what the planners printed before they moved into the header (when each read the override
and the kernel rate itself): the move changed no plan.  The GPU tests then check the bytes the plans render."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-sdr-gps-sim_amd", "csrc")

# planner and configuration: the result without the override | with it at 0 | 1 | 2 | 3 | 5 | 8 | 40 | -1
# (pieces as their sizes, "size x count" for a run; fixed: the nominal piece, "one" where the call takes one piece;
# reference: chunk, "kb" where kernel-bound, the head of a chain on the device)
EXPECTED = """\
d2h nsamp=260000 ss=1: 65 | 0 | 1 | 2 | 3 | 5 | 8 | 40 | 0
d2h nsamp=260000 ss=2: 33 | 0 | 1 | 2 | 3 | 5 | 8 | 40 | 0
d2h nsamp=1000000 ss=1: 17 | 0 | 1 | 2 | 3 | 5 | 8 | 40 | 0
d2h nsamp=1000000 ss=2: 9 | 0 | 1 | 2 | 3 | 5 | 8 | 40 | 0
d2h nsamp=2500000 ss=1: 8 | 0 | 1 | 2 | 3 | 5 | 8 | 40 | 0
d2h nsamp=2500000 ss=2: 8 | 0 | 1 | 2 | 3 | 5 | 8 | 40 | 0
d2h nsamp=33333 ss=1: 504 | 0 | 1 | 2 | 3 | 5 | 8 | 40 | 0
d2h nsamp=33333 ss=2: 252 | 0 | 1 | 2 | 3 | 5 | 8 | 40 | 0
kernel_bound nsamp=260000 nchan=12 rate=6e+12 threads=16: 0
kernel_bound nsamp=260000 nchan=12 rate=6e+12 threads=4: 0
kernel_bound nsamp=260000 nchan=12 rate=1.5e+12 threads=16: 0
kernel_bound nsamp=260000 nchan=12 rate=1.5e+12 threads=4: 0
kernel_bound nsamp=260000 nchan=16 rate=6e+12 threads=16: 0
kernel_bound nsamp=260000 nchan=16 rate=6e+12 threads=4: 0
kernel_bound nsamp=260000 nchan=16 rate=1.5e+12 threads=16: 0
kernel_bound nsamp=260000 nchan=16 rate=1.5e+12 threads=4: 0
kernel_bound nsamp=1000000 nchan=12 rate=6e+12 threads=16: 0
kernel_bound nsamp=1000000 nchan=12 rate=6e+12 threads=4: 0
kernel_bound nsamp=1000000 nchan=12 rate=1.5e+12 threads=16: 1
kernel_bound nsamp=1000000 nchan=12 rate=1.5e+12 threads=4: 0
kernel_bound nsamp=1000000 nchan=16 rate=6e+12 threads=16: 0
kernel_bound nsamp=1000000 nchan=16 rate=6e+12 threads=4: 0
kernel_bound nsamp=1000000 nchan=16 rate=1.5e+12 threads=16: 1
kernel_bound nsamp=1000000 nchan=16 rate=1.5e+12 threads=4: 0
kernel_bound nsamp=2500000 nchan=12 rate=6e+12 threads=16: 0
kernel_bound nsamp=2500000 nchan=12 rate=6e+12 threads=4: 0
kernel_bound nsamp=2500000 nchan=12 rate=1.5e+12 threads=16: 1
kernel_bound nsamp=2500000 nchan=12 rate=1.5e+12 threads=4: 0
kernel_bound nsamp=2500000 nchan=16 rate=6e+12 threads=16: 0
kernel_bound nsamp=2500000 nchan=16 rate=6e+12 threads=4: 0
kernel_bound nsamp=2500000 nchan=16 rate=1.5e+12 threads=16: 1
kernel_bound nsamp=2500000 nchan=16 rate=1.5e+12 threads=4: 0
fixed nsamp=260000 nblocks=1: 1 one | 1 one | 1 one | 1 one | 1 one | 1 one | 1 one | 1 one | 1 one
fixed nsamp=260000 nblocks=100: 100 one | 100 one | 1 1 2 4 9 16x5 4 | 2 1 2 4 9 16x5 4 | 3 1 2 4 9 16x5 4 | 5 1 2 4 9 16x5 4 | 8 1 2 4 9 16x5 4 | 40 2 4 9 20 44 21 | 100 one
fixed nsamp=260000 nblocks=211: 211 one | 211 one | 1 1 2 4 9 16x12 3 | 2 1 2 4 9 16x12 3 | 3 1 2 4 9 16x12 3 | 5 1 2 4 9 16x12 3 | 8 1 2 4 9 16x12 3 | 40 2 4 9 20 44 80 52 | 211 one
fixed nsamp=260000 nblocks=212: 212 one | 212 one | 1 1 2 4 9 16x12 4 | 2 1 2 4 9 16x12 4 | 3 1 2 4 9 16x12 4 | 5 1 2 4 9 16x12 4 | 8 1 2 4 9 16x12 4 | 40 2 4 9 20 44 80 53 | 212 one
fixed nsamp=260000 nblocks=531: 531 one | 531 one | 1 1 2 4 9 16x32 3 | 2 1 2 4 9 16x32 3 | 3 1 2 4 9 16x32 3 | 5 1 2 4 9 16x32 3 | 8 1 2 4 9 16x32 3 | 40 2 4 9 20 44 80x5 52 | 531 one
fixed nsamp=260000 nblocks=532: 532 one | 532 one | 1 1 2 4 9 16x32 4 | 2 1 2 4 9 16x32 4 | 3 1 2 4 9 16x32 4 | 5 1 2 4 9 16x32 4 | 8 1 2 4 9 16x32 4 | 40 2 4 9 20 44 80x5 53 | 532 one
fixed nsamp=260000 nblocks=2047: 2047 one | 2047 one | 1 1 2 4 9 16x126 15 | 2 1 2 4 9 16x126 15 | 3 1 2 4 9 16x126 15 | 5 1 2 4 9 16x126 15 | 8 1 2 4 9 16x126 15 | 40 2 4 9 20 44 80x24 48 | 2047 one
fixed nsamp=260000 nblocks=2048: 1024 64 141 310 682 851 | 2048 one | 1 1 2 4 9 16x127 | 2 1 2 4 9 16x127 | 3 1 2 4 9 16x127 | 5 1 2 4 9 16x127 | 8 1 2 4 9 16x127 | 40 2 4 9 20 44 80x24 49 | 2048 one
fixed nsamp=260000 nblocks=4000: 1024 64 141 310 682 1500 1303 | 4000 one | 1 1 2 4 9 16x249 | 2 1 2 4 9 16x249 | 3 1 2 4 9 16x249 | 5 1 2 4 9 16x249 | 8 1 2 4 9 16x249 | 40 2 4 9 20 44 80x48 81 | 4000 one
fixed nsamp=1000000 nblocks=1: 1 one | 1 one | 1 one | 1 one | 1 one | 1 one | 1 one | 1 one | 1 one
fixed nsamp=1000000 nblocks=100: 100 one | 100 one | 1 1 2 4 9 16x5 4 | 2 1 2 4 9 16x5 4 | 3 1 2 4 9 16x5 4 | 5 1 2 4 9 16x5 4 | 8 1 2 4 9 16x5 4 | 40 2 4 9 20 44 21 | 100 one
fixed nsamp=1000000 nblocks=211: 211 one | 211 one | 1 1 2 4 9 16x12 3 | 2 1 2 4 9 16x12 3 | 3 1 2 4 9 16x12 3 | 5 1 2 4 9 16x12 3 | 8 1 2 4 9 16x12 3 | 40 2 4 9 20 44 80 52 | 211 one
fixed nsamp=1000000 nblocks=212: 212 one | 212 one | 1 1 2 4 9 16x12 4 | 2 1 2 4 9 16x12 4 | 3 1 2 4 9 16x12 4 | 5 1 2 4 9 16x12 4 | 8 1 2 4 9 16x12 4 | 40 2 4 9 20 44 80 53 | 212 one
fixed nsamp=1000000 nblocks=531: 531 one | 531 one | 1 1 2 4 9 16x32 3 | 2 1 2 4 9 16x32 3 | 3 1 2 4 9 16x32 3 | 5 1 2 4 9 16x32 3 | 8 1 2 4 9 16x32 3 | 40 2 4 9 20 44 80x5 52 | 531 one
fixed nsamp=1000000 nblocks=532: 266 16 35 77 169 235 | 532 one | 1 1 2 4 9 16x32 4 | 2 1 2 4 9 16x32 4 | 3 1 2 4 9 16x32 4 | 5 1 2 4 9 16x32 4 | 8 1 2 4 9 16x32 4 | 40 2 4 9 20 44 80x5 53 | 532 one
fixed nsamp=1000000 nblocks=2047: 266 16 35 77 169 372 528x2 322 | 2047 one | 1 1 2 4 9 16x126 15 | 2 1 2 4 9 16x126 15 | 3 1 2 4 9 16x126 15 | 5 1 2 4 9 16x126 15 | 8 1 2 4 9 16x126 15 | 40 2 4 9 20 44 80x24 48 | 2047 one
fixed nsamp=1000000 nblocks=2048: 266 16 35 77 169 372 528x2 323 | 2048 one | 1 1 2 4 9 16x127 | 2 1 2 4 9 16x127 | 3 1 2 4 9 16x127 | 5 1 2 4 9 16x127 | 8 1 2 4 9 16x127 | 40 2 4 9 20 44 80x24 49 | 2048 one
fixed nsamp=1000000 nblocks=4000: 266 16 35 77 169 372 528x6 163 | 4000 one | 1 1 2 4 9 16x249 | 2 1 2 4 9 16x249 | 3 1 2 4 9 16x249 | 5 1 2 4 9 16x249 | 8 1 2 4 9 16x249 | 40 2 4 9 20 44 80x48 81 | 4000 one
fixed nsamp=2500000 nblocks=1: 1 one | 1 one | 1 one | 1 one | 1 one | 1 one | 1 one | 1 one | 1 one
fixed nsamp=2500000 nblocks=100: 100 one | 100 one | 1 1 2 4 9 16x5 4 | 2 1 2 4 9 16x5 4 | 3 1 2 4 9 16x5 4 | 5 1 2 4 9 16x5 4 | 8 1 2 4 9 16x5 4 | 40 2 4 9 20 44 21 | 100 one
fixed nsamp=2500000 nblocks=211: 211 one | 211 one | 1 1 2 4 9 16x12 3 | 2 1 2 4 9 16x12 3 | 3 1 2 4 9 16x12 3 | 5 1 2 4 9 16x12 3 | 8 1 2 4 9 16x12 3 | 40 2 4 9 20 44 80 52 | 211 one
fixed nsamp=2500000 nblocks=212: 106 6 13 29 64 100 | 212 one | 1 1 2 4 9 16x12 4 | 2 1 2 4 9 16x12 4 | 3 1 2 4 9 16x12 4 | 5 1 2 4 9 16x12 4 | 8 1 2 4 9 16x12 4 | 40 2 4 9 20 44 80 53 | 212 one
fixed nsamp=2500000 nblocks=531: 106 6 13 29 64 141 208 70 | 531 one | 1 1 2 4 9 16x32 3 | 2 1 2 4 9 16x32 3 | 3 1 2 4 9 16x32 3 | 5 1 2 4 9 16x32 3 | 8 1 2 4 9 16x32 3 | 40 2 4 9 20 44 80x5 52 | 531 one
fixed nsamp=2500000 nblocks=532: 106 6 13 29 64 141 208 71 | 532 one | 1 1 2 4 9 16x32 4 | 2 1 2 4 9 16x32 4 | 3 1 2 4 9 16x32 4 | 5 1 2 4 9 16x32 4 | 8 1 2 4 9 16x32 4 | 40 2 4 9 20 44 80x5 53 | 532 one
fixed nsamp=2500000 nblocks=2047: 106 6 13 29 64 141 208x8 130 | 2047 one | 1 1 2 4 9 16x126 15 | 2 1 2 4 9 16x126 15 | 3 1 2 4 9 16x126 15 | 5 1 2 4 9 16x126 15 | 8 1 2 4 9 16x126 15 | 40 2 4 9 20 44 80x24 48 | 2047 one
fixed nsamp=2500000 nblocks=2048: 106 6 13 29 64 141 208x8 131 | 2048 one | 1 1 2 4 9 16x127 | 2 1 2 4 9 16x127 | 3 1 2 4 9 16x127 | 5 1 2 4 9 16x127 | 8 1 2 4 9 16x127 | 40 2 4 9 20 44 80x24 49 | 2048 one
fixed nsamp=2500000 nblocks=4000: 106 6 13 29 64 141 208x17 211 | 4000 one | 1 1 2 4 9 16x249 | 2 1 2 4 9 16x249 | 3 1 2 4 9 16x249 | 5 1 2 4 9 16x249 | 8 1 2 4 9 16x249 | 40 2 4 9 20 44 80x48 81 | 4000 one
reference nsamp=260000 nchan=12 rate=6e+12 nblocks=1: 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1
reference nsamp=260000 nchan=12 rate=6e+12 nblocks=40: 40 head=40 40 | 40 head=40 40 | 1 head=40 1x2 2x18 1x2 | 2 head=40 1 2 4x8 2x2 1 | 3 head=40 1 3 6x4 8 3 1 | 5 head=40 2 5 10x2 6 5 2 | 8 head=40 4 8 16 8 4 | 40 head=40 40 | 40 head=40 40
reference nsamp=260000 nchan=12 rate=6e+12 nblocks=1024: 256 head=1024 256x4 | 1024 head=1024 1024 | 1 head=1024 1x2 2x510 1x2 | 2 head=1024 1 2 4x254 2x2 1 | 3 head=1024 1 3 6x168 8 3 1 | 5 head=1024 2 5 10x101 5 2 | 8 head=1024 4 8 16x62 8x2 4 | 40 head=1024 20 40 80x10 104 40 20 | 1024 head=1024 1024
reference nsamp=260000 nchan=12 rate=6e+12 nblocks=1025: 256 head=1025 128 256 257 256 128 | 1025 head=1025 1025 | 1 head=1025 1x2 2x510 1x3 | 2 head=1025 1 2 4x254 3 2 1 | 3 head=1025 1 3 6x169 3x2 1 | 5 head=1025 2 5 10x100 11 5 2 | 8 head=1025 4 8 16x62 9 8 4 | 40 head=1025 20 40 80x10 105 40 20 | 1025 head=1025 1025
reference nsamp=260000 nchan=12 rate=6e+12 nblocks=1200: 256 head=1200 128 256 432 256 128 | 1200 head=1200 1200 | 1 head=1200 1x2 2x598 1x2 | 2 head=1200 1 2 4x298 2x2 1 | 3 head=1200 1 3 6x198 4 3 1 | 5 head=1200 2 5 10x118 6 5 2 | 8 head=1200 4 8 16x73 8x2 4 | 40 head=1200 20 40 80x13 40x2 20 | 1200 head=1200 1200
reference nsamp=260000 nchan=12 rate=6e+12 nblocks=3000: 256 head=896 128 256 512x3 696 256 128 | 3000 head=3000 3000 | 1 head=770 1x2 2x1498 1x2 | 2 head=771 1 2 4x748 2x2 1 | 3 head=772 1 3 6x498 4 3 1 | 5 head=777 2 5 10x298 6 5 2 | 8 head=780 4 8 16x186 8 4 | 40 head=780 20 40 80x36 40 20 | 3000 head=3000 3000
reference nsamp=260000 nchan=12 rate=1.5e+12 nblocks=1: 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1
reference nsamp=260000 nchan=12 rate=1.5e+12 nblocks=40: 40 head=40 40 | 40 head=40 40 | 1 head=40 1x2 2x18 1x2 | 2 head=40 1 2 4x8 2x2 1 | 3 head=40 1 3 6x4 8 3 1 | 5 head=40 2 5 10x2 6 5 2 | 8 head=40 4 8 16 8 4 | 40 head=40 40 | 40 head=40 40
reference nsamp=260000 nchan=12 rate=1.5e+12 nblocks=1024: 256 head=256 256x4 | 1024 head=1024 1024 | 1 head=194 1x2 2x510 1x2 | 2 head=195 1 2 4x254 2x2 1 | 3 head=196 1 3 6x168 8 3 1 | 5 head=197 2 5 10x101 5 2 | 8 head=204 4 8 16x62 8x2 4 | 40 head=220 20 40 80x10 104 40 20 | 1024 head=1024 1024
reference nsamp=260000 nchan=12 rate=1.5e+12 nblocks=1025: 256 head=384 128 256 257 256 128 | 1025 head=1025 1025 | 1 head=194 1x2 2x510 1x3 | 2 head=195 1 2 4x254 3 2 1 | 3 head=196 1 3 6x169 3x2 1 | 5 head=197 2 5 10x100 11 5 2 | 8 head=204 4 8 16x62 9 8 4 | 40 head=220 20 40 80x10 105 40 20 | 1025 head=1025 1025
reference nsamp=260000 nchan=12 rate=1.5e+12 nblocks=1200: 256 head=384 128 256 432 256 128 | 1200 head=1200 1200 | 1 head=194 1x2 2x598 1x2 | 2 head=195 1 2 4x298 2x2 1 | 3 head=196 1 3 6x198 4 3 1 | 5 head=197 2 5 10x118 6 5 2 | 8 head=204 4 8 16x73 8x2 4 | 40 head=220 20 40 80x13 40x2 20 | 1200 head=1200 1200
reference nsamp=260000 nchan=12 rate=1.5e+12 nblocks=3000: 256 head=384 128 256 512x3 696 256 128 | 3000 head=3000 3000 | 1 head=194 1x2 2x1498 1x2 | 2 head=195 1 2 4x748 2x2 1 | 3 head=196 1 3 6x498 4 3 1 | 5 head=197 2 5 10x298 6 5 2 | 8 head=204 4 8 16x186 8 4 | 40 head=220 20 40 80x36 40 20 | 3000 head=3000 3000
reference nsamp=260000 nchan=16 rate=6e+12 nblocks=1: 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1
reference nsamp=260000 nchan=16 rate=6e+12 nblocks=40: 40 head=40 40 | 40 head=40 40 | 1 head=40 1x2 2x18 1x2 | 2 head=40 1 2 4x8 2x2 1 | 3 head=40 1 3 6x4 8 3 1 | 5 head=40 2 5 10x2 6 5 2 | 8 head=40 4 8 16 8 4 | 40 head=40 40 | 40 head=40 40
reference nsamp=260000 nchan=16 rate=6e+12 nblocks=1024: 256 head=1024 256x4 | 1024 head=1024 1024 | 1 head=1024 1x2 2x510 1x2 | 2 head=1024 1 2 4x254 2x2 1 | 3 head=1024 1 3 6x168 8 3 1 | 5 head=1024 2 5 10x101 5 2 | 8 head=1024 4 8 16x62 8x2 4 | 40 head=1024 20 40 80x10 104 40 20 | 1024 head=1024 1024
reference nsamp=260000 nchan=16 rate=6e+12 nblocks=1025: 256 head=1025 128 256 257 256 128 | 1025 head=1025 1025 | 1 head=1025 1x2 2x510 1x3 | 2 head=1025 1 2 4x254 3 2 1 | 3 head=1025 1 3 6x169 3x2 1 | 5 head=1025 2 5 10x100 11 5 2 | 8 head=1025 4 8 16x62 9 8 4 | 40 head=1025 20 40 80x10 105 40 20 | 1025 head=1025 1025
reference nsamp=260000 nchan=16 rate=6e+12 nblocks=1200: 256 head=1200 128 256 432 256 128 | 1200 head=1200 1200 | 1 head=578 1x2 2x598 1x2 | 2 head=579 1 2 4x298 2x2 1 | 3 head=580 1 3 6x198 4 3 1 | 5 head=577 2 5 10x118 6 5 2 | 8 head=588 4 8 16x73 8x2 4 | 40 head=1200 20 40 80x13 40x2 20 | 1200 head=1200 1200
reference nsamp=260000 nchan=16 rate=6e+12 nblocks=3000: 256 head=896 128 256 512x3 696 256 128 | 3000 head=3000 3000 | 1 head=578 1x2 2x1498 1x2 | 2 head=579 1 2 4x748 2x2 1 | 3 head=580 1 3 6x498 4 3 1 | 5 head=577 2 5 10x298 6 5 2 | 8 head=588 4 8 16x186 8 4 | 40 head=620 20 40 80x36 40 20 | 3000 head=3000 3000
reference nsamp=260000 nchan=16 rate=1.5e+12 nblocks=1: 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1
reference nsamp=260000 nchan=16 rate=1.5e+12 nblocks=40: 40 head=40 40 | 40 head=40 40 | 1 head=40 1x2 2x18 1x2 | 2 head=40 1 2 4x8 2x2 1 | 3 head=40 1 3 6x4 8 3 1 | 5 head=40 2 5 10x2 6 5 2 | 8 head=40 4 8 16 8 4 | 40 head=40 40 | 40 head=40 40
reference nsamp=260000 nchan=16 rate=1.5e+12 nblocks=1024: 256 head=256 256x4 | 1024 head=1024 1024 | 1 head=146 1x2 2x510 1x2 | 2 head=147 1 2 4x254 2x2 1 | 3 head=148 1 3 6x168 8 3 1 | 5 head=147 2 5 10x101 5 2 | 8 head=156 4 8 16x62 8x2 4 | 40 head=220 20 40 80x10 104 40 20 | 1024 head=1024 1024
reference nsamp=260000 nchan=16 rate=1.5e+12 nblocks=1025: 256 head=384 128 256 257 256 128 | 1025 head=1025 1025 | 1 head=146 1x2 2x510 1x3 | 2 head=147 1 2 4x254 3 2 1 | 3 head=148 1 3 6x169 3x2 1 | 5 head=147 2 5 10x100 11 5 2 | 8 head=156 4 8 16x62 9 8 4 | 40 head=220 20 40 80x10 105 40 20 | 1025 head=1025 1025
reference nsamp=260000 nchan=16 rate=1.5e+12 nblocks=1200: 256 head=384 128 256 432 256 128 | 1200 head=1200 1200 | 1 head=146 1x2 2x598 1x2 | 2 head=147 1 2 4x298 2x2 1 | 3 head=148 1 3 6x198 4 3 1 | 5 head=147 2 5 10x118 6 5 2 | 8 head=156 4 8 16x73 8x2 4 | 40 head=220 20 40 80x13 40x2 20 | 1200 head=1200 1200
reference nsamp=260000 nchan=16 rate=1.5e+12 nblocks=3000: 256 head=384 128 256 512x3 696 256 128 | 3000 head=3000 3000 | 1 head=146 1x2 2x1498 1x2 | 2 head=147 1 2 4x748 2x2 1 | 3 head=148 1 3 6x498 4 3 1 | 5 head=147 2 5 10x298 6 5 2 | 8 head=156 4 8 16x186 8 4 | 40 head=220 20 40 80x36 40 20 | 3000 head=3000 3000
reference nsamp=1000000 nchan=12 rate=6e+12 nblocks=1: 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1
reference nsamp=1000000 nchan=12 rate=6e+12 nblocks=40: 40 head=40 40 | 40 head=40 40 | 1 head=40 1x2 2x18 1x2 | 2 head=40 1 2 4x8 2x2 1 | 3 head=40 1 3 6x4 8 3 1 | 5 head=40 2 5 10x2 6 5 2 | 8 head=40 4 8 16 8 4 | 40 head=40 40 | 40 head=40 40
reference nsamp=1000000 nchan=12 rate=6e+12 nblocks=264: 66 head=264 66x4 | 264 head=264 264 | 1 head=264 1x2 2x130 1x2 | 2 head=264 1 2 4x64 2x2 1 | 3 head=264 1 3 6x42 4 3 1 | 5 head=264 2 5 10x25 5 2 | 8 head=264 4 8 16x15 8 4 | 40 head=264 20 40 80 64 40 20 | 264 head=264 264
reference nsamp=1000000 nchan=12 rate=6e+12 nblocks=265: 66 head=265 33 66 67 66 33 | 265 head=265 265 | 1 head=265 1x2 2x130 1x3 | 2 head=265 1 2 4x64 3 2 1 | 3 head=265 1 3 6x42 5 3 1 | 5 head=265 2 5 10x24 11 5 2 | 8 head=265 4 8 16x14 17 8 4 | 40 head=265 20 40 80 65 40 20 | 265 head=265 265
reference nsamp=1000000 nchan=12 rate=6e+12 nblocks=1200: 66 head=231 33 66 132x7 78 66 33 | 1200 head=1200 1200 | 1 head=202 1x2 2x598 1x2 | 2 head=203 1 2 4x298 2x2 1 | 3 head=202 1 3 6x198 4 3 1 | 5 head=207 2 5 10x118 6 5 2 | 8 head=204 4 8 16x73 8x2 4 | 40 head=220 20 40 80x13 40x2 20 | 1200 head=1200 1200
reference nsamp=1000000 nchan=12 rate=6e+12 nblocks=3000: 66 head=231 33 66 132x20 162 66 33 | 3000 head=3000 3000 | 1 head=202 1x2 2x1498 1x2 | 2 head=203 1 2 4x748 2x2 1 | 3 head=202 1 3 6x498 4 3 1 | 5 head=207 2 5 10x298 6 5 2 | 8 head=204 4 8 16x186 8 4 | 40 head=220 20 40 80x36 40 20 | 3000 head=3000 3000
reference nsamp=1000000 nchan=12 rate=1.5e+12 nblocks=1: 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1
reference nsamp=1000000 nchan=12 rate=1.5e+12 nblocks=40: 40 kb head=40 40 | 40 kb head=40 40 | 1 kb head=40 1 2 4 9 16 8 | 2 kb head=40 1 2 4 9 20 4 | 3 kb head=40 1 2 4 9 20 4 | 5 kb head=40 2 4 9 20 5 | 8 kb head=40 4 9 20 7 | 40 kb head=40 40 | 40 kb head=40 40
reference nsamp=1000000 nchan=12 rate=1.5e+12 nblocks=264: 66 kb head=66 66x4 | 264 kb head=264 264 | 1 kb head=64 1 2 4 9 16x15 8 | 2 kb head=68 1 2 4 9 20 32x7 4 | 3 kb head=80 1 2 4 9 20 44 48x3 40 | 5 kb head=79 2 4 9 20 44 80x2 25 | 8 kb head=77 4 9 20 44 97 90 | 40 kb head=64 20 44 97 103 | 264 kb head=264 264
reference nsamp=1000000 nchan=12 rate=1.5e+12 nblocks=265: 66 kb head=106 33 73 159 | 265 kb head=265 265 | 1 kb head=64 1 2 4 9 16x15 9 | 2 kb head=68 1 2 4 9 20 32x7 5 | 3 kb head=80 1 2 4 9 20 44 48x3 41 | 5 kb head=79 2 4 9 20 44 80x2 26 | 8 kb head=77 4 9 20 44 97 91 | 40 kb head=64 20 44 97 104 | 265 kb head=265 265
reference nsamp=1000000 nchan=12 rate=1.5e+12 nblocks=1200: 66 kb head=106 33 73 161 354 579 | 1200 kb head=1200 1200 | 1 kb head=64 1 2 4 9 16x74 | 2 kb head=68 1 2 4 9 20 32x36 12 | 3 kb head=80 1 2 4 9 20 44 48x23 16 | 5 kb head=79 2 4 9 20 44 80x13 81 | 8 kb head=77 4 9 20 44 97 128x7 130 | 40 kb head=64 20 44 97 213 469 357 | 1200 kb head=1200 1200
reference nsamp=1000000 nchan=12 rate=1.5e+12 nblocks=3000: 66 kb head=106 33 73 161 354 779 1056 544 | 3000 kb head=3000 3000 | 1 kb head=64 1 2 4 9 16x186 8 | 2 kb head=68 1 2 4 9 20 32x92 20 | 3 kb head=80 1 2 4 9 20 44 48x60 40 | 5 kb head=79 2 4 9 20 44 80x36 41 | 8 kb head=77 4 9 20 44 97 128x22 10 | 40 kb head=64 20 44 97 213 469 640x3 237 | 3000 kb head=3000 3000
reference nsamp=1000000 nchan=16 rate=6e+12 nblocks=1: 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1
reference nsamp=1000000 nchan=16 rate=6e+12 nblocks=40: 40 head=40 40 | 40 head=40 40 | 1 head=40 1x2 2x18 1x2 | 2 head=40 1 2 4x8 2x2 1 | 3 head=40 1 3 6x4 8 3 1 | 5 head=40 2 5 10x2 6 5 2 | 8 head=40 4 8 16 8 4 | 40 head=40 40 | 40 head=40 40
reference nsamp=1000000 nchan=16 rate=6e+12 nblocks=264: 66 head=264 66x4 | 264 head=264 264 | 1 head=264 1x2 2x130 1x2 | 2 head=264 1 2 4x64 2x2 1 | 3 head=264 1 3 6x42 4 3 1 | 5 head=264 2 5 10x25 5 2 | 8 head=264 4 8 16x15 8 4 | 40 head=264 20 40 80 64 40 20 | 264 head=264 264
reference nsamp=1000000 nchan=16 rate=6e+12 nblocks=265: 66 head=265 33 66 67 66 33 | 265 head=265 265 | 1 head=265 1x2 2x130 1x3 | 2 head=265 1 2 4x64 3 2 1 | 3 head=265 1 3 6x42 5 3 1 | 5 head=265 2 5 10x24 11 5 2 | 8 head=265 4 8 16x14 17 8 4 | 40 head=265 20 40 80 65 40 20 | 265 head=265 265
reference nsamp=1000000 nchan=16 rate=6e+12 nblocks=1200: 66 head=231 33 66 132x7 78 66 33 | 1200 head=1200 1200 | 1 head=152 1x2 2x598 1x2 | 2 head=151 1 2 4x298 2x2 1 | 3 head=154 1 3 6x198 4 3 1 | 5 head=157 2 5 10x118 6 5 2 | 8 head=156 4 8 16x73 8x2 4 | 40 head=220 20 40 80x13 40x2 20 | 1200 head=1200 1200
reference nsamp=1000000 nchan=16 rate=6e+12 nblocks=3000: 66 head=231 33 66 132x20 162 66 33 | 3000 head=3000 3000 | 1 head=152 1x2 2x1498 1x2 | 2 head=151 1 2 4x748 2x2 1 | 3 head=154 1 3 6x498 4 3 1 | 5 head=157 2 5 10x298 6 5 2 | 8 head=156 4 8 16x186 8 4 | 40 head=220 20 40 80x36 40 20 | 3000 head=3000 3000
reference nsamp=1000000 nchan=16 rate=1.5e+12 nblocks=1: 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1
reference nsamp=1000000 nchan=16 rate=1.5e+12 nblocks=40: 40 kb head=40 40 | 40 kb head=40 40 | 1 kb head=40 1 2 4 9 16 8 | 2 kb head=40 1 2 4 9 20 4 | 3 kb head=40 1 2 4 9 20 4 | 5 kb head=40 2 4 9 20 5 | 8 kb head=40 4 9 20 7 | 40 kb head=40 40 | 40 kb head=40 40
reference nsamp=1000000 nchan=16 rate=1.5e+12 nblocks=264: 66 kb head=66 66x4 | 264 kb head=264 264 | 1 kb head=48 1 2 4 9 16x15 8 | 2 kb head=68 1 2 4 9 20 32x7 4 | 3 kb head=80 1 2 4 9 20 44 48x3 40 | 5 kb head=79 2 4 9 20 44 80x2 25 | 8 kb head=77 4 9 20 44 97 90 | 40 kb head=64 20 44 97 103 | 264 kb head=264 264
reference nsamp=1000000 nchan=16 rate=1.5e+12 nblocks=265: 66 kb head=106 33 73 159 | 265 kb head=265 265 | 1 kb head=48 1 2 4 9 16x15 9 | 2 kb head=68 1 2 4 9 20 32x7 5 | 3 kb head=80 1 2 4 9 20 44 48x3 41 | 5 kb head=79 2 4 9 20 44 80x2 26 | 8 kb head=77 4 9 20 44 97 91 | 40 kb head=64 20 44 97 104 | 265 kb head=265 265
reference nsamp=1000000 nchan=16 rate=1.5e+12 nblocks=1200: 66 kb head=106 33 73 161 354 579 | 1200 kb head=1200 1200 | 1 kb head=48 1 2 4 9 16x74 | 2 kb head=68 1 2 4 9 20 32x36 12 | 3 kb head=80 1 2 4 9 20 44 48x23 16 | 5 kb head=79 2 4 9 20 44 80x13 81 | 8 kb head=77 4 9 20 44 97 128x7 130 | 40 kb head=64 20 44 97 213 469 357 | 1200 kb head=1200 1200
reference nsamp=1000000 nchan=16 rate=1.5e+12 nblocks=3000: 66 kb head=106 33 73 161 354 779 1056 544 | 3000 kb head=3000 3000 | 1 kb head=48 1 2 4 9 16x186 8 | 2 kb head=68 1 2 4 9 20 32x92 20 | 3 kb head=80 1 2 4 9 20 44 48x60 40 | 5 kb head=79 2 4 9 20 44 80x36 41 | 8 kb head=77 4 9 20 44 97 128x22 10 | 40 kb head=64 20 44 97 213 469 640x3 237 | 3000 kb head=3000 3000
reference nsamp=2500000 nchan=12 rate=6e+12 nblocks=1: 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1
reference nsamp=2500000 nchan=12 rate=6e+12 nblocks=40: 26 head=40 26 14 | 40 head=40 40 | 1 head=40 1x2 2x18 1x2 | 2 head=40 1 2 4x8 2x2 1 | 3 head=40 1 3 6x4 8 3 1 | 5 head=40 2 5 10x2 6 5 2 | 8 head=40 4 8 16 8 4 | 40 head=40 40 | 40 head=40 40
reference nsamp=2500000 nchan=12 rate=6e+12 nblocks=104: 26 head=104 26x4 | 104 head=104 104 | 1 head=104 1x2 2x50 1x2 | 2 head=104 1 2 4x24 2x2 1 | 3 head=104 1 3 6x16 3 1 | 5 head=104 2 5 10x9 5 2 | 8 head=104 4 8 16x5 8 4 | 40 head=104 40x2 24 | 104 head=104 104
reference nsamp=2500000 nchan=12 rate=6e+12 nblocks=105: 26 head=105 13 26 27 26 13 | 105 head=105 105 | 1 head=105 1x2 2x50 1x3 | 2 head=105 1 2 4x24 3 2 1 | 3 head=105 1 3 6x15 7 3 1 | 5 head=105 2 5 10x8 11 5 2 | 8 head=105 4 8 16x4 17 8 4 | 40 head=105 40x2 25 | 105 head=105 105
reference nsamp=2500000 nchan=12 rate=6e+12 nblocks=1200: 26 head=91 13 26 52x21 30 26 13 | 1200 head=1200 1200 | 1 head=82 1x2 2x598 1x2 | 2 head=83 1 2 4x298 2x2 1 | 3 head=82 1 3 6x198 4 3 1 | 5 head=87 2 5 10x118 6 5 2 | 8 head=92 4 8 16x73 8x2 4 | 40 head=140 20 40 80x13 40x2 20 | 1200 head=1200 1200
reference nsamp=2500000 nchan=12 rate=6e+12 nblocks=3000: 26 head=91 13 26 52x55 62 26 13 | 3000 head=3000 3000 | 1 head=82 1x2 2x1498 1x2 | 2 head=83 1 2 4x748 2x2 1 | 3 head=82 1 3 6x498 4 3 1 | 5 head=87 2 5 10x298 6 5 2 | 8 head=92 4 8 16x186 8 4 | 40 head=140 20 40 80x36 40 20 | 3000 head=3000 3000
reference nsamp=2500000 nchan=12 rate=1.5e+12 nblocks=1: 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1
reference nsamp=2500000 nchan=12 rate=1.5e+12 nblocks=40: 26 kb head=40 26 14 | 40 kb head=40 40 | 1 kb head=40 1 2 4 9 16 8 | 2 kb head=40 1 2 4 9 20 4 | 3 kb head=40 1 2 4 9 20 4 | 5 kb head=40 2 4 9 20 5 | 8 kb head=40 4 9 20 7 | 40 kb head=40 40 | 40 kb head=40 40
reference nsamp=2500000 nchan=12 rate=1.5e+12 nblocks=104: 26 kb head=26 26x4 | 104 kb head=104 104 | 1 kb head=32 1 2 4 9 16x5 8 | 2 kb head=36 1 2 4 9 20 32x2 4 | 3 kb head=36 1 2 4 9 20 44 24 | 5 kb head=35 2 4 9 20 44 25 | 8 kb head=33 4 9 20 44 27 | 40 kb head=40 40x2 24 | 104 kb head=104 104
reference nsamp=2500000 nchan=12 rate=1.5e+12 nblocks=105: 26 kb head=42 13 29 63 | 105 kb head=105 105 | 1 kb head=32 1 2 4 9 16x5 9 | 2 kb head=36 1 2 4 9 20 32x2 5 | 3 kb head=36 1 2 4 9 20 44 25 | 5 kb head=35 2 4 9 20 44 26 | 8 kb head=33 4 9 20 44 28 | 40 kb head=40 40x2 25 | 105 kb head=105 105
reference nsamp=2500000 nchan=12 rate=1.5e+12 nblocks=1200: 26 kb head=42 13 29 64 141 310 416 227 | 1200 kb head=1200 1200 | 1 kb head=32 1 2 4 9 16x74 | 2 kb head=36 1 2 4 9 20 32x36 12 | 3 kb head=36 1 2 4 9 20 44 48x23 16 | 5 kb head=35 2 4 9 20 44 80x13 81 | 8 kb head=33 4 9 20 44 97 128x7 130 | 40 kb head=64 20 44 97 213 469 357 | 1200 kb head=1200 1200
reference nsamp=2500000 nchan=12 rate=1.5e+12 nblocks=3000: 26 kb head=42 13 29 64 141 310 416x5 363 | 3000 kb head=3000 3000 | 1 kb head=32 1 2 4 9 16x186 8 | 2 kb head=36 1 2 4 9 20 32x92 20 | 3 kb head=36 1 2 4 9 20 44 48x60 40 | 5 kb head=35 2 4 9 20 44 80x36 41 | 8 kb head=33 4 9 20 44 97 128x22 10 | 40 kb head=64 20 44 97 213 469 640x3 237 | 3000 kb head=3000 3000
reference nsamp=2500000 nchan=16 rate=6e+12 nblocks=1: 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1 | 1 head=1 1
reference nsamp=2500000 nchan=16 rate=6e+12 nblocks=40: 26 head=40 26 14 | 40 head=40 40 | 1 head=40 1x2 2x18 1x2 | 2 head=40 1 2 4x8 2x2 1 | 3 head=40 1 3 6x4 8 3 1 | 5 head=40 2 5 10x2 6 5 2 | 8 head=40 4 8 16 8 4 | 40 head=40 40 | 40 head=40 40
reference nsamp=2500000 nchan=16 rate=6e+12 nblocks=104: 26 head=104 26x4 | 104 head=104 104 | 1 head=104 1x2 2x50 1x2 | 2 head=104 1 2 4x24 2x2 1 | 3 head=104 1 3 6x16 3 1 | 5 head=104 2 5 10x9 5 2 | 8 head=104 4 8 16x5 8 4 | 40 head=104 40x2 24 | 104 head=104 104
reference nsamp=2500000 nchan=16 rate=6e+12 nblocks=105: 26 head=105 13 26 27 26 13 | 105 head=105 105 | 1 head=105 1x2 2x50 1x3 | 2 head=105 1 2 4x24 3 2 1 | 3 head=105 1 3 6x15 7 3 1 | 5 head=105 2 5 10x8 11 5 2 | 8 head=105 4 8 16x4 17 8 4 | 40 head=105 40x2 25 | 105 head=105 105
reference nsamp=2500000 nchan=16 rate=6e+12 nblocks=1200: 26 head=91 13 26 52x21 30 26 13 | 1200 head=1200 1200 | 1 head=62 1x2 2x598 1x2 | 2 head=63 1 2 4x298 2x2 1 | 3 head=64 1 3 6x198 4 3 1 | 5 head=67 2 5 10x118 6 5 2 | 8 head=76 4 8 16x73 8x2 4 | 40 head=140 20 40 80x13 40x2 20 | 1200 head=1200 1200
reference nsamp=2500000 nchan=16 rate=6e+12 nblocks=3000: 26 head=91 13 26 52x55 62 26 13 | 3000 head=3000 3000 | 1 head=62 1x2 2x1498 1x2 | 2 head=63 1 2 4x748 2x2 1 | 3 head=64 1 3 6x498 4 3 1 | 5 head=67 2 5 10x298 6 5 2 | 8 head=76 4 8 16x186 8 4 | 40 head=140 20 40 80x36 40 20 | 3000 head=3000 3000
reference nsamp=2500000 nchan=16 rate=1.5e+12 nblocks=1: 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1 | 1 kb head=1 1
reference nsamp=2500000 nchan=16 rate=1.5e+12 nblocks=40: 26 kb head=40 26 14 | 40 kb head=40 40 | 1 kb head=16 1 2 4 9 16 8 | 2 kb head=16 1 2 4 9 20 4 | 3 kb head=16 1 2 4 9 20 4 | 5 kb head=40 2 4 9 20 5 | 8 kb head=40 4 9 20 7 | 40 kb head=40 40 | 40 kb head=40 40
reference nsamp=2500000 nchan=16 rate=1.5e+12 nblocks=104: 26 kb head=26 26x4 | 104 kb head=104 104 | 1 kb head=16 1 2 4 9 16x5 8 | 2 kb head=16 1 2 4 9 20 32x2 4 | 3 kb head=16 1 2 4 9 20 44 24 | 5 kb head=35 2 4 9 20 44 25 | 8 kb head=33 4 9 20 44 27 | 40 kb head=40 40x2 24 | 104 kb head=104 104
reference nsamp=2500000 nchan=16 rate=1.5e+12 nblocks=105: 26 kb head=42 13 29 63 | 105 kb head=105 105 | 1 kb head=16 1 2 4 9 16x5 9 | 2 kb head=16 1 2 4 9 20 32x2 5 | 3 kb head=16 1 2 4 9 20 44 25 | 5 kb head=35 2 4 9 20 44 26 | 8 kb head=33 4 9 20 44 28 | 40 kb head=40 40x2 25 | 105 kb head=105 105
reference nsamp=2500000 nchan=16 rate=1.5e+12 nblocks=1200: 26 kb head=42 13 29 64 141 310 416 227 | 1200 kb head=1200 1200 | 1 kb head=16 1 2 4 9 16x74 | 2 kb head=16 1 2 4 9 20 32x36 12 | 3 kb head=16 1 2 4 9 20 44 48x23 16 | 5 kb head=35 2 4 9 20 44 80x13 81 | 8 kb head=33 4 9 20 44 97 128x7 130 | 40 kb head=20 20 44 97 213 469 357 | 1200 kb head=1200 1200
reference nsamp=2500000 nchan=16 rate=1.5e+12 nblocks=3000: 26 kb head=42 13 29 64 141 310 416x5 363 | 3000 kb head=3000 3000 | 1 kb head=16 1 2 4 9 16x186 8 | 2 kb head=16 1 2 4 9 20 32x92 20 | 3 kb head=16 1 2 4 9 20 44 48x60 40 | 5 kb head=35 2 4 9 20 44 80x36 41 | 8 kb head=33 4 9 20 44 97 128x22 10 | 40 kb head=20 20 44 97 213 469 640x3 237 | 3000 kb head=3000 3000
reference ranges nsamp=260000 0-700 700-1400: 256x2 188 256x2 188 | 700x2 | 1x2 2x348 1x4 2x348 1x2 | 1 2 4x173 2x2 1x2 2 4x173 2x2 1 | 1 3 6x114 8 3 1x2 3 6x114 8 3 1 | 2 5 10x68 6 5 2x2 5 10x68 6 5 2 | 4 8 16x41 20 8 4x2 8 16x41 20 8 4 | 20 40 80x6 100 40 20x2 40 80x6 100 40 20 | 700x2
reference ranges nsamp=1000000 0-700 700-1400: 33 66 132x3 106 66 33x2 66 132x3 106 66 33 | 700x2 | 1x2 2x348 1x4 2x348 1x2 | 1 2 4x173 2x2 1x2 2 4x173 2x2 1 | 1 3 6x114 8 3 1x2 3 6x114 8 3 1 | 2 5 10x68 6 5 2x2 5 10x68 6 5 2 | 4 8 16x41 20 8 4x2 8 16x41 20 8 4 | 20 40 80x6 100 40 20x2 40 80x6 100 40 20 | 700x2
reference ranges nsamp=2500000 0-700 700-1400: 13 26 52x11 50 26 13x2 26 52x11 50 26 13 | 700x2 | 1x2 2x348 1x4 2x348 1x2 | 1 2 4x173 2x2 1x2 2 4x173 2x2 1 | 1 3 6x114 8 3 1x2 3 6x114 8 3 1 | 2 5 10x68 6 5 2x2 5 10x68 6 5 2 | 4 8 16x41 20 8 4x2 8 16x41 20 8 4 | 20 40 80x6 100 40 20x2 40 80x6 100 40 20 | 700x2
device nsamp=260000 nchan=12 host_rows=0 reference=0 nblocks=1: 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1
device nsamp=260000 nchan=12 host_rows=0 reference=0 nblocks=31: 31 | 31 | 1 8 22 | 2 16 13 | 3 28 | 5 26 | 8 23 | 31 | 31
device nsamp=260000 nchan=12 host_rows=0 reference=0 nblocks=32: 32 | 32 | 1 8 23 | 2 16 14 | 3 29 | 5 27 | 8 24 | 32 | 32
device nsamp=260000 nchan=12 host_rows=0 reference=0 nblocks=33: 33 | 33 | 1 8 24 | 2 16 15 | 3 30 | 5 28 | 8 25 | 33 | 33
device nsamp=260000 nchan=12 host_rows=0 reference=0 nblocks=200: 200 | 200 | 1 8 64 127 | 2 16 182 | 3 24 173 | 5 40 155 | 8 64 128 | 40 160 | 200
device nsamp=260000 nchan=12 host_rows=0 reference=0 nblocks=1100: 1100 | 1100 | 1 8 64 512 515 | 2 16 128 954 | 3 24 192 881 | 5 40 320 735 | 8 64 512 516 | 40 320 740 | 1100
device nsamp=260000 nchan=12 host_rows=0 reference=0 nblocks=30000: 30000 | 30000 | 1 8 64 512 4096 25319 | 2 16 128 1024 8192 20638 | 3 24 192 1536 12288 15957 | 5 40 320 2560 27075 | 8 64 512 4096 25320 | 40 320 2560 27080 | 30000
device nsamp=260000 nchan=12 host_rows=0 reference=0 nblocks=1000000: 1000000 | 1000000 | 1 8 64 512 4096 32768 262144 700407 | 2 16 128 1024 8192 65536 524288 400814 | 3 24 192 1536 12288 98304 887653 | 5 40 320 2560 20480 163840 812755 | 8 64 512 4096 32768 262144 700408 | 40 320 2560 20480 163840 812760 | 1000000
device nsamp=260000 nchan=12 host_rows=0 reference=1 nblocks=1: 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1
device nsamp=260000 nchan=12 host_rows=0 reference=1 nblocks=31: 31 | 31 | 1 8 22 | 2 16 13 | 3 28 | 5 26 | 8 23 | 31 | 31
device nsamp=260000 nchan=12 host_rows=0 reference=1 nblocks=32: 32 | 32 | 1 8 23 | 2 16 14 | 3 29 | 5 27 | 8 24 | 32 | 32
device nsamp=260000 nchan=12 host_rows=0 reference=1 nblocks=33: 33 | 33 | 1 8 24 | 2 16 15 | 3 30 | 5 28 | 8 25 | 33 | 33
device nsamp=260000 nchan=12 host_rows=0 reference=1 nblocks=200: 200 | 200 | 1 8 64 127 | 2 16 182 | 3 24 173 | 5 40 155 | 8 64 128 | 40 160 | 200
device nsamp=260000 nchan=12 host_rows=0 reference=1 nblocks=1100: 289 811 | 1100 | 1 8 64 512 515 | 2 16 128 954 | 3 24 192 881 | 5 40 320 735 | 8 64 512 516 | 40 320 740 | 1100
device nsamp=260000 nchan=12 host_rows=0 reference=1 nblocks=30000: 289 2312 27399 | 30000 | 1 8 64 512 4096 25319 | 2 16 128 1024 8192 20638 | 3 24 192 1536 12288 15957 | 5 40 320 2560 27075 | 8 64 512 4096 25320 | 40 320 2560 27080 | 30000
device nsamp=260000 nchan=12 host_rows=0 reference=1 nblocks=1000000: 289 2312 18496 147968 830935 | 1000000 | 1 8 64 512 4096 32768 262144 700407 | 2 16 128 1024 8192 65536 524288 400814 | 3 24 192 1536 12288 98304 887653 | 5 40 320 2560 20480 163840 812755 | 8 64 512 4096 32768 262144 700408 | 40 320 2560 20480 163840 812760 | 1000000
device nsamp=260000 nchan=12 host_rows=1 reference=0 nblocks=1: 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1
device nsamp=260000 nchan=12 host_rows=1 reference=0 nblocks=31: 31 | 31 | 1 8 22 | 2 16 13 | 3 28 | 5 26 | 8 23 | 31 | 31
device nsamp=260000 nchan=12 host_rows=1 reference=0 nblocks=32: 32 | 32 | 1 8 23 | 2 16 14 | 3 29 | 5 27 | 8 24 | 32 | 32
device nsamp=260000 nchan=12 host_rows=1 reference=0 nblocks=33: 33 | 33 | 1 8 24 | 2 16 15 | 3 30 | 5 28 | 8 25 | 33 | 33
device nsamp=260000 nchan=12 host_rows=1 reference=0 nblocks=200: 200 | 200 | 1 8 64 127 | 2 16 182 | 3 24 173 | 5 40 155 | 8 64 128 | 40 160 | 200
device nsamp=260000 nchan=12 host_rows=1 reference=0 nblocks=1100: 1100 | 1100 | 1 8 64 512 515 | 2 16 128 954 | 3 24 192 881 | 5 40 320 735 | 8 64 512 516 | 40 320 740 | 1100
device nsamp=260000 nchan=12 host_rows=1 reference=0 nblocks=30000: 674 5392 23934 | 30000 | 1 8 64 512 4096 25319 | 2 16 128 1024 8192 20638 | 3 24 192 1536 12288 15957 | 5 40 320 2560 27075 | 8 64 512 4096 25320 | 40 320 2560 27080 | 30000
device nsamp=260000 nchan=12 host_rows=1 reference=0 nblocks=1000000: 674 5392 43136 345088 605710 | 1000000 | 1 8 64 512 4096 32768 262144 700407 | 2 16 128 1024 8192 65536 524288 400814 | 3 24 192 1536 12288 98304 887653 | 5 40 320 2560 20480 163840 812755 | 8 64 512 4096 32768 262144 700408 | 40 320 2560 20480 163840 812760 | 1000000
device nsamp=260000 nchan=12 host_rows=1 reference=1 nblocks=1: 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1
device nsamp=260000 nchan=12 host_rows=1 reference=1 nblocks=31: 31 | 31 | 1 8 22 | 2 16 13 | 3 28 | 5 26 | 8 23 | 31 | 31
device nsamp=260000 nchan=12 host_rows=1 reference=1 nblocks=32: 32 | 32 | 1 8 23 | 2 16 14 | 3 29 | 5 27 | 8 24 | 32 | 32
device nsamp=260000 nchan=12 host_rows=1 reference=1 nblocks=33: 33 | 33 | 1 8 24 | 2 16 15 | 3 30 | 5 28 | 8 25 | 33 | 33
device nsamp=260000 nchan=12 host_rows=1 reference=1 nblocks=200: 200 | 200 | 1 8 64 127 | 2 16 182 | 3 24 173 | 5 40 155 | 8 64 128 | 40 160 | 200
device nsamp=260000 nchan=12 host_rows=1 reference=1 nblocks=1100: 1100 | 1100 | 1 8 64 512 515 | 2 16 128 954 | 3 24 192 881 | 5 40 320 735 | 8 64 512 516 | 40 320 740 | 1100
device nsamp=260000 nchan=12 host_rows=1 reference=1 nblocks=30000: 674 5392 23934 | 30000 | 1 8 64 512 4096 25319 | 2 16 128 1024 8192 20638 | 3 24 192 1536 12288 15957 | 5 40 320 2560 27075 | 8 64 512 4096 25320 | 40 320 2560 27080 | 30000
device nsamp=260000 nchan=12 host_rows=1 reference=1 nblocks=1000000: 674 5392 43136 345088 605710 | 1000000 | 1 8 64 512 4096 32768 262144 700407 | 2 16 128 1024 8192 65536 524288 400814 | 3 24 192 1536 12288 98304 887653 | 5 40 320 2560 20480 163840 812755 | 8 64 512 4096 32768 262144 700408 | 40 320 2560 20480 163840 812760 | 1000000
device nsamp=260000 nchan=16 host_rows=0 reference=0 nblocks=1: 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1
device nsamp=260000 nchan=16 host_rows=0 reference=0 nblocks=31: 31 | 31 | 1 8 22 | 2 16 13 | 3 28 | 5 26 | 8 23 | 31 | 31
device nsamp=260000 nchan=16 host_rows=0 reference=0 nblocks=32: 32 | 32 | 1 8 23 | 2 16 14 | 3 29 | 5 27 | 8 24 | 32 | 32
device nsamp=260000 nchan=16 host_rows=0 reference=0 nblocks=33: 33 | 33 | 1 8 24 | 2 16 15 | 3 30 | 5 28 | 8 25 | 33 | 33
device nsamp=260000 nchan=16 host_rows=0 reference=0 nblocks=200: 200 | 200 | 1 8 64 127 | 2 16 182 | 3 24 173 | 5 40 155 | 8 64 128 | 40 160 | 200
device nsamp=260000 nchan=16 host_rows=0 reference=0 nblocks=1100: 1100 | 1100 | 1 8 64 512 515 | 2 16 128 954 | 3 24 192 881 | 5 40 320 735 | 8 64 512 516 | 40 320 740 | 1100
device nsamp=260000 nchan=16 host_rows=0 reference=0 nblocks=30000: 30000 | 30000 | 1 8 64 512 4096 25319 | 2 16 128 1024 8192 20638 | 3 24 192 1536 12288 15957 | 5 40 320 2560 27075 | 8 64 512 4096 25320 | 40 320 2560 27080 | 30000
device nsamp=260000 nchan=16 host_rows=0 reference=0 nblocks=1000000: 1000000 | 1000000 | 1 8 64 512 4096 32768 262144 700407 | 2 16 128 1024 8192 65536 524288 400814 | 3 24 192 1536 12288 98304 887653 | 5 40 320 2560 20480 163840 812755 | 8 64 512 4096 32768 262144 700408 | 40 320 2560 20480 163840 812760 | 1000000
device nsamp=260000 nchan=16 host_rows=0 reference=1 nblocks=1: 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1
device nsamp=260000 nchan=16 host_rows=0 reference=1 nblocks=31: 31 | 31 | 1 8 22 | 2 16 13 | 3 28 | 5 26 | 8 23 | 31 | 31
device nsamp=260000 nchan=16 host_rows=0 reference=1 nblocks=32: 32 | 32 | 1 8 23 | 2 16 14 | 3 29 | 5 27 | 8 24 | 32 | 32
device nsamp=260000 nchan=16 host_rows=0 reference=1 nblocks=33: 33 | 33 | 1 8 24 | 2 16 15 | 3 30 | 5 28 | 8 25 | 33 | 33
device nsamp=260000 nchan=16 host_rows=0 reference=1 nblocks=200: 200 | 200 | 1 8 64 127 | 2 16 182 | 3 24 173 | 5 40 155 | 8 64 128 | 40 160 | 200
device nsamp=260000 nchan=16 host_rows=0 reference=1 nblocks=1100: 217 883 | 1100 | 1 8 64 512 515 | 2 16 128 954 | 3 24 192 881 | 5 40 320 735 | 8 64 512 516 | 40 320 740 | 1100
device nsamp=260000 nchan=16 host_rows=0 reference=1 nblocks=30000: 217 1736 13888 14159 | 30000 | 1 8 64 512 4096 25319 | 2 16 128 1024 8192 20638 | 3 24 192 1536 12288 15957 | 5 40 320 2560 27075 | 8 64 512 4096 25320 | 40 320 2560 27080 | 30000
device nsamp=260000 nchan=16 host_rows=0 reference=1 nblocks=1000000: 217 1736 13888 111104 873055 | 1000000 | 1 8 64 512 4096 32768 262144 700407 | 2 16 128 1024 8192 65536 524288 400814 | 3 24 192 1536 12288 98304 887653 | 5 40 320 2560 20480 163840 812755 | 8 64 512 4096 32768 262144 700408 | 40 320 2560 20480 163840 812760 | 1000000
device nsamp=260000 nchan=16 host_rows=1 reference=0 nblocks=1: 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1
device nsamp=260000 nchan=16 host_rows=1 reference=0 nblocks=31: 31 | 31 | 1 8 22 | 2 16 13 | 3 28 | 5 26 | 8 23 | 31 | 31
device nsamp=260000 nchan=16 host_rows=1 reference=0 nblocks=32: 32 | 32 | 1 8 23 | 2 16 14 | 3 29 | 5 27 | 8 24 | 32 | 32
device nsamp=260000 nchan=16 host_rows=1 reference=0 nblocks=33: 33 | 33 | 1 8 24 | 2 16 15 | 3 30 | 5 28 | 8 25 | 33 | 33
device nsamp=260000 nchan=16 host_rows=1 reference=0 nblocks=200: 200 | 200 | 1 8 64 127 | 2 16 182 | 3 24 173 | 5 40 155 | 8 64 128 | 40 160 | 200
device nsamp=260000 nchan=16 host_rows=1 reference=0 nblocks=1100: 505 595 | 1100 | 1 8 64 512 515 | 2 16 128 954 | 3 24 192 881 | 5 40 320 735 | 8 64 512 516 | 40 320 740 | 1100
device nsamp=260000 nchan=16 host_rows=1 reference=0 nblocks=30000: 505 4040 25455 | 30000 | 1 8 64 512 4096 25319 | 2 16 128 1024 8192 20638 | 3 24 192 1536 12288 15957 | 5 40 320 2560 27075 | 8 64 512 4096 25320 | 40 320 2560 27080 | 30000
device nsamp=260000 nchan=16 host_rows=1 reference=0 nblocks=1000000: 505 4040 32320 258560 704575 | 1000000 | 1 8 64 512 4096 32768 262144 700407 | 2 16 128 1024 8192 65536 524288 400814 | 3 24 192 1536 12288 98304 887653 | 5 40 320 2560 20480 163840 812755 | 8 64 512 4096 32768 262144 700408 | 40 320 2560 20480 163840 812760 | 1000000
device nsamp=260000 nchan=16 host_rows=1 reference=1 nblocks=1: 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1
device nsamp=260000 nchan=16 host_rows=1 reference=1 nblocks=31: 31 | 31 | 1 8 22 | 2 16 13 | 3 28 | 5 26 | 8 23 | 31 | 31
device nsamp=260000 nchan=16 host_rows=1 reference=1 nblocks=32: 32 | 32 | 1 8 23 | 2 16 14 | 3 29 | 5 27 | 8 24 | 32 | 32
device nsamp=260000 nchan=16 host_rows=1 reference=1 nblocks=33: 33 | 33 | 1 8 24 | 2 16 15 | 3 30 | 5 28 | 8 25 | 33 | 33
device nsamp=260000 nchan=16 host_rows=1 reference=1 nblocks=200: 200 | 200 | 1 8 64 127 | 2 16 182 | 3 24 173 | 5 40 155 | 8 64 128 | 40 160 | 200
device nsamp=260000 nchan=16 host_rows=1 reference=1 nblocks=1100: 505 595 | 1100 | 1 8 64 512 515 | 2 16 128 954 | 3 24 192 881 | 5 40 320 735 | 8 64 512 516 | 40 320 740 | 1100
device nsamp=260000 nchan=16 host_rows=1 reference=1 nblocks=30000: 505 4040 25455 | 30000 | 1 8 64 512 4096 25319 | 2 16 128 1024 8192 20638 | 3 24 192 1536 12288 15957 | 5 40 320 2560 27075 | 8 64 512 4096 25320 | 40 320 2560 27080 | 30000
device nsamp=260000 nchan=16 host_rows=1 reference=1 nblocks=1000000: 505 4040 32320 258560 704575 | 1000000 | 1 8 64 512 4096 32768 262144 700407 | 2 16 128 1024 8192 65536 524288 400814 | 3 24 192 1536 12288 98304 887653 | 5 40 320 2560 20480 163840 812755 | 8 64 512 4096 32768 262144 700408 | 40 320 2560 20480 163840 812760 | 1000000
device nsamp=1000000 nchan=12 host_rows=0 reference=0 nblocks=1: 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1
device nsamp=1000000 nchan=12 host_rows=0 reference=0 nblocks=31: 31 | 31 | 1 8 22 | 2 16 13 | 3 28 | 5 26 | 8 23 | 31 | 31
device nsamp=1000000 nchan=12 host_rows=0 reference=0 nblocks=32: 32 | 32 | 1 8 23 | 2 16 14 | 3 29 | 5 27 | 8 24 | 32 | 32
device nsamp=1000000 nchan=12 host_rows=0 reference=0 nblocks=33: 33 | 33 | 1 8 24 | 2 16 15 | 3 30 | 5 28 | 8 25 | 33 | 33
device nsamp=1000000 nchan=12 host_rows=0 reference=0 nblocks=200: 200 | 200 | 1 8 64 127 | 2 16 182 | 3 24 173 | 5 40 155 | 8 64 128 | 40 160 | 200
device nsamp=1000000 nchan=12 host_rows=0 reference=0 nblocks=1100: 1100 | 1100 | 1 8 64 512 515 | 2 16 128 954 | 3 24 192 881 | 5 40 320 735 | 8 64 512 516 | 40 320 740 | 1100
device nsamp=1000000 nchan=12 host_rows=0 reference=0 nblocks=30000: 30000 | 30000 | 1 8 64 512 4096 25319 | 2 16 128 1024 8192 20638 | 3 24 192 1536 12288 15957 | 5 40 320 2560 27075 | 8 64 512 4096 25320 | 40 320 2560 27080 | 30000
device nsamp=1000000 nchan=12 host_rows=0 reference=0 nblocks=1000000: 1000000 | 1000000 | 1 8 64 512 4096 32768 262144 700407 | 2 16 128 1024 8192 65536 524288 400814 | 3 24 192 1536 12288 98304 887653 | 5 40 320 2560 20480 163840 812755 | 8 64 512 4096 32768 262144 700408 | 40 320 2560 20480 163840 812760 | 1000000
device nsamp=1000000 nchan=12 host_rows=0 reference=1 nblocks=1: 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1
device nsamp=1000000 nchan=12 host_rows=0 reference=1 nblocks=31: 31 | 31 | 1 8 22 | 2 16 13 | 3 28 | 5 26 | 8 23 | 31 | 31
device nsamp=1000000 nchan=12 host_rows=0 reference=1 nblocks=32: 32 | 32 | 1 8 23 | 2 16 14 | 3 29 | 5 27 | 8 24 | 32 | 32
device nsamp=1000000 nchan=12 host_rows=0 reference=1 nblocks=33: 33 | 33 | 1 8 24 | 2 16 15 | 3 30 | 5 28 | 8 25 | 33 | 33
device nsamp=1000000 nchan=12 host_rows=0 reference=1 nblocks=200: 76 124 | 200 | 1 8 64 127 | 2 16 182 | 3 24 173 | 5 40 155 | 8 64 128 | 40 160 | 200
device nsamp=1000000 nchan=12 host_rows=0 reference=1 nblocks=1100: 76 608 416 | 1100 | 1 8 64 512 515 | 2 16 128 954 | 3 24 192 881 | 5 40 320 735 | 8 64 512 516 | 40 320 740 | 1100
device nsamp=1000000 nchan=12 host_rows=0 reference=1 nblocks=30000: 76 608 4864 24452 | 30000 | 1 8 64 512 4096 25319 | 2 16 128 1024 8192 20638 | 3 24 192 1536 12288 15957 | 5 40 320 2560 27075 | 8 64 512 4096 25320 | 40 320 2560 27080 | 30000
device nsamp=1000000 nchan=12 host_rows=0 reference=1 nblocks=1000000: 76 608 4864 38912 311296 644244 | 1000000 | 1 8 64 512 4096 32768 262144 700407 | 2 16 128 1024 8192 65536 524288 400814 | 3 24 192 1536 12288 98304 887653 | 5 40 320 2560 20480 163840 812755 | 8 64 512 4096 32768 262144 700408 | 40 320 2560 20480 163840 812760 | 1000000
device nsamp=1000000 nchan=12 host_rows=1 reference=0 nblocks=1: 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1
device nsamp=1000000 nchan=12 host_rows=1 reference=0 nblocks=31: 31 | 31 | 1 8 22 | 2 16 13 | 3 28 | 5 26 | 8 23 | 31 | 31
device nsamp=1000000 nchan=12 host_rows=1 reference=0 nblocks=32: 32 | 32 | 1 8 23 | 2 16 14 | 3 29 | 5 27 | 8 24 | 32 | 32
device nsamp=1000000 nchan=12 host_rows=1 reference=0 nblocks=33: 33 | 33 | 1 8 24 | 2 16 15 | 3 30 | 5 28 | 8 25 | 33 | 33
device nsamp=1000000 nchan=12 host_rows=1 reference=0 nblocks=200: 200 | 200 | 1 8 64 127 | 2 16 182 | 3 24 173 | 5 40 155 | 8 64 128 | 40 160 | 200
device nsamp=1000000 nchan=12 host_rows=1 reference=0 nblocks=1100: 176 924 | 1100 | 1 8 64 512 515 | 2 16 128 954 | 3 24 192 881 | 5 40 320 735 | 8 64 512 516 | 40 320 740 | 1100
device nsamp=1000000 nchan=12 host_rows=1 reference=0 nblocks=30000: 176 1408 11264 17152 | 30000 | 1 8 64 512 4096 25319 | 2 16 128 1024 8192 20638 | 3 24 192 1536 12288 15957 | 5 40 320 2560 27075 | 8 64 512 4096 25320 | 40 320 2560 27080 | 30000
device nsamp=1000000 nchan=12 host_rows=1 reference=0 nblocks=1000000: 176 1408 11264 90112 897040 | 1000000 | 1 8 64 512 4096 32768 262144 700407 | 2 16 128 1024 8192 65536 524288 400814 | 3 24 192 1536 12288 98304 887653 | 5 40 320 2560 20480 163840 812755 | 8 64 512 4096 32768 262144 700408 | 40 320 2560 20480 163840 812760 | 1000000
device nsamp=1000000 nchan=12 host_rows=1 reference=1 nblocks=1: 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1
device nsamp=1000000 nchan=12 host_rows=1 reference=1 nblocks=31: 31 | 31 | 1 8 22 | 2 16 13 | 3 28 | 5 26 | 8 23 | 31 | 31
device nsamp=1000000 nchan=12 host_rows=1 reference=1 nblocks=32: 32 | 32 | 1 8 23 | 2 16 14 | 3 29 | 5 27 | 8 24 | 32 | 32
device nsamp=1000000 nchan=12 host_rows=1 reference=1 nblocks=33: 33 | 33 | 1 8 24 | 2 16 15 | 3 30 | 5 28 | 8 25 | 33 | 33
device nsamp=1000000 nchan=12 host_rows=1 reference=1 nblocks=200: 200 | 200 | 1 8 64 127 | 2 16 182 | 3 24 173 | 5 40 155 | 8 64 128 | 40 160 | 200
device nsamp=1000000 nchan=12 host_rows=1 reference=1 nblocks=1100: 176 924 | 1100 | 1 8 64 512 515 | 2 16 128 954 | 3 24 192 881 | 5 40 320 735 | 8 64 512 516 | 40 320 740 | 1100
device nsamp=1000000 nchan=12 host_rows=1 reference=1 nblocks=30000: 176 1408 11264 17152 | 30000 | 1 8 64 512 4096 25319 | 2 16 128 1024 8192 20638 | 3 24 192 1536 12288 15957 | 5 40 320 2560 27075 | 8 64 512 4096 25320 | 40 320 2560 27080 | 30000
device nsamp=1000000 nchan=12 host_rows=1 reference=1 nblocks=1000000: 176 1408 11264 90112 897040 | 1000000 | 1 8 64 512 4096 32768 262144 700407 | 2 16 128 1024 8192 65536 524288 400814 | 3 24 192 1536 12288 98304 887653 | 5 40 320 2560 20480 163840 812755 | 8 64 512 4096 32768 262144 700408 | 40 320 2560 20480 163840 812760 | 1000000
device nsamp=1000000 nchan=16 host_rows=0 reference=0 nblocks=1: 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1
device nsamp=1000000 nchan=16 host_rows=0 reference=0 nblocks=31: 31 | 31 | 1 8 22 | 2 16 13 | 3 28 | 5 26 | 8 23 | 31 | 31
device nsamp=1000000 nchan=16 host_rows=0 reference=0 nblocks=32: 32 | 32 | 1 8 23 | 2 16 14 | 3 29 | 5 27 | 8 24 | 32 | 32
device nsamp=1000000 nchan=16 host_rows=0 reference=0 nblocks=33: 33 | 33 | 1 8 24 | 2 16 15 | 3 30 | 5 28 | 8 25 | 33 | 33
device nsamp=1000000 nchan=16 host_rows=0 reference=0 nblocks=200: 200 | 200 | 1 8 64 127 | 2 16 182 | 3 24 173 | 5 40 155 | 8 64 128 | 40 160 | 200
device nsamp=1000000 nchan=16 host_rows=0 reference=0 nblocks=1100: 1100 | 1100 | 1 8 64 512 515 | 2 16 128 954 | 3 24 192 881 | 5 40 320 735 | 8 64 512 516 | 40 320 740 | 1100
device nsamp=1000000 nchan=16 host_rows=0 reference=0 nblocks=30000: 30000 | 30000 | 1 8 64 512 4096 25319 | 2 16 128 1024 8192 20638 | 3 24 192 1536 12288 15957 | 5 40 320 2560 27075 | 8 64 512 4096 25320 | 40 320 2560 27080 | 30000
device nsamp=1000000 nchan=16 host_rows=0 reference=0 nblocks=1000000: 1000000 | 1000000 | 1 8 64 512 4096 32768 262144 700407 | 2 16 128 1024 8192 65536 524288 400814 | 3 24 192 1536 12288 98304 887653 | 5 40 320 2560 20480 163840 812755 | 8 64 512 4096 32768 262144 700408 | 40 320 2560 20480 163840 812760 | 1000000
device nsamp=1000000 nchan=16 host_rows=0 reference=1 nblocks=1: 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1
device nsamp=1000000 nchan=16 host_rows=0 reference=1 nblocks=31: 31 | 31 | 1 8 22 | 2 16 13 | 3 28 | 5 26 | 8 23 | 31 | 31
device nsamp=1000000 nchan=16 host_rows=0 reference=1 nblocks=32: 32 | 32 | 1 8 23 | 2 16 14 | 3 29 | 5 27 | 8 24 | 32 | 32
device nsamp=1000000 nchan=16 host_rows=0 reference=1 nblocks=33: 33 | 33 | 1 8 24 | 2 16 15 | 3 30 | 5 28 | 8 25 | 33 | 33
device nsamp=1000000 nchan=16 host_rows=0 reference=1 nblocks=200: 57 143 | 200 | 1 8 64 127 | 2 16 182 | 3 24 173 | 5 40 155 | 8 64 128 | 40 160 | 200
device nsamp=1000000 nchan=16 host_rows=0 reference=1 nblocks=1100: 57 456 587 | 1100 | 1 8 64 512 515 | 2 16 128 954 | 3 24 192 881 | 5 40 320 735 | 8 64 512 516 | 40 320 740 | 1100
device nsamp=1000000 nchan=16 host_rows=0 reference=1 nblocks=30000: 57 456 3648 25839 | 30000 | 1 8 64 512 4096 25319 | 2 16 128 1024 8192 20638 | 3 24 192 1536 12288 15957 | 5 40 320 2560 27075 | 8 64 512 4096 25320 | 40 320 2560 27080 | 30000
device nsamp=1000000 nchan=16 host_rows=0 reference=1 nblocks=1000000: 57 456 3648 29184 233472 733183 | 1000000 | 1 8 64 512 4096 32768 262144 700407 | 2 16 128 1024 8192 65536 524288 400814 | 3 24 192 1536 12288 98304 887653 | 5 40 320 2560 20480 163840 812755 | 8 64 512 4096 32768 262144 700408 | 40 320 2560 20480 163840 812760 | 1000000
device nsamp=1000000 nchan=16 host_rows=1 reference=0 nblocks=1: 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1
device nsamp=1000000 nchan=16 host_rows=1 reference=0 nblocks=31: 31 | 31 | 1 8 22 | 2 16 13 | 3 28 | 5 26 | 8 23 | 31 | 31
device nsamp=1000000 nchan=16 host_rows=1 reference=0 nblocks=32: 32 | 32 | 1 8 23 | 2 16 14 | 3 29 | 5 27 | 8 24 | 32 | 32
device nsamp=1000000 nchan=16 host_rows=1 reference=0 nblocks=33: 33 | 33 | 1 8 24 | 2 16 15 | 3 30 | 5 28 | 8 25 | 33 | 33
device nsamp=1000000 nchan=16 host_rows=1 reference=0 nblocks=200: 200 | 200 | 1 8 64 127 | 2 16 182 | 3 24 173 | 5 40 155 | 8 64 128 | 40 160 | 200
device nsamp=1000000 nchan=16 host_rows=1 reference=0 nblocks=1100: 132 968 | 1100 | 1 8 64 512 515 | 2 16 128 954 | 3 24 192 881 | 5 40 320 735 | 8 64 512 516 | 40 320 740 | 1100
device nsamp=1000000 nchan=16 host_rows=1 reference=0 nblocks=30000: 132 1056 8448 20364 | 30000 | 1 8 64 512 4096 25319 | 2 16 128 1024 8192 20638 | 3 24 192 1536 12288 15957 | 5 40 320 2560 27075 | 8 64 512 4096 25320 | 40 320 2560 27080 | 30000
device nsamp=1000000 nchan=16 host_rows=1 reference=0 nblocks=1000000: 132 1056 8448 67584 540672 382108 | 1000000 | 1 8 64 512 4096 32768 262144 700407 | 2 16 128 1024 8192 65536 524288 400814 | 3 24 192 1536 12288 98304 887653 | 5 40 320 2560 20480 163840 812755 | 8 64 512 4096 32768 262144 700408 | 40 320 2560 20480 163840 812760 | 1000000
device nsamp=1000000 nchan=16 host_rows=1 reference=1 nblocks=1: 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1
device nsamp=1000000 nchan=16 host_rows=1 reference=1 nblocks=31: 31 | 31 | 1 8 22 | 2 16 13 | 3 28 | 5 26 | 8 23 | 31 | 31
device nsamp=1000000 nchan=16 host_rows=1 reference=1 nblocks=32: 32 | 32 | 1 8 23 | 2 16 14 | 3 29 | 5 27 | 8 24 | 32 | 32
device nsamp=1000000 nchan=16 host_rows=1 reference=1 nblocks=33: 33 | 33 | 1 8 24 | 2 16 15 | 3 30 | 5 28 | 8 25 | 33 | 33
device nsamp=1000000 nchan=16 host_rows=1 reference=1 nblocks=200: 200 | 200 | 1 8 64 127 | 2 16 182 | 3 24 173 | 5 40 155 | 8 64 128 | 40 160 | 200
device nsamp=1000000 nchan=16 host_rows=1 reference=1 nblocks=1100: 132 968 | 1100 | 1 8 64 512 515 | 2 16 128 954 | 3 24 192 881 | 5 40 320 735 | 8 64 512 516 | 40 320 740 | 1100
device nsamp=1000000 nchan=16 host_rows=1 reference=1 nblocks=30000: 132 1056 8448 20364 | 30000 | 1 8 64 512 4096 25319 | 2 16 128 1024 8192 20638 | 3 24 192 1536 12288 15957 | 5 40 320 2560 27075 | 8 64 512 4096 25320 | 40 320 2560 27080 | 30000
device nsamp=1000000 nchan=16 host_rows=1 reference=1 nblocks=1000000: 132 1056 8448 67584 540672 382108 | 1000000 | 1 8 64 512 4096 32768 262144 700407 | 2 16 128 1024 8192 65536 524288 400814 | 3 24 192 1536 12288 98304 887653 | 5 40 320 2560 20480 163840 812755 | 8 64 512 4096 32768 262144 700408 | 40 320 2560 20480 163840 812760 | 1000000
device nsamp=2500000 nchan=12 host_rows=0 reference=0 nblocks=1: 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1
device nsamp=2500000 nchan=12 host_rows=0 reference=0 nblocks=31: 31 | 31 | 1 8 22 | 2 16 13 | 3 28 | 5 26 | 8 23 | 31 | 31
device nsamp=2500000 nchan=12 host_rows=0 reference=0 nblocks=32: 32 | 32 | 1 8 23 | 2 16 14 | 3 29 | 5 27 | 8 24 | 32 | 32
device nsamp=2500000 nchan=12 host_rows=0 reference=0 nblocks=33: 33 | 33 | 1 8 24 | 2 16 15 | 3 30 | 5 28 | 8 25 | 33 | 33
device nsamp=2500000 nchan=12 host_rows=0 reference=0 nblocks=200: 200 | 200 | 1 8 64 127 | 2 16 182 | 3 24 173 | 5 40 155 | 8 64 128 | 40 160 | 200
device nsamp=2500000 nchan=12 host_rows=0 reference=0 nblocks=1100: 1100 | 1100 | 1 8 64 512 515 | 2 16 128 954 | 3 24 192 881 | 5 40 320 735 | 8 64 512 516 | 40 320 740 | 1100
device nsamp=2500000 nchan=12 host_rows=0 reference=0 nblocks=30000: 30000 | 30000 | 1 8 64 512 4096 25319 | 2 16 128 1024 8192 20638 | 3 24 192 1536 12288 15957 | 5 40 320 2560 27075 | 8 64 512 4096 25320 | 40 320 2560 27080 | 30000
device nsamp=2500000 nchan=12 host_rows=0 reference=0 nblocks=1000000: 1000000 | 1000000 | 1 8 64 512 4096 32768 262144 700407 | 2 16 128 1024 8192 65536 524288 400814 | 3 24 192 1536 12288 98304 887653 | 5 40 320 2560 20480 163840 812755 | 8 64 512 4096 32768 262144 700408 | 40 320 2560 20480 163840 812760 | 1000000
device nsamp=2500000 nchan=12 host_rows=0 reference=1 nblocks=1: 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1
device nsamp=2500000 nchan=12 host_rows=0 reference=1 nblocks=31: 31 | 31 | 1 8 22 | 2 16 13 | 3 28 | 5 26 | 8 23 | 31 | 31
device nsamp=2500000 nchan=12 host_rows=0 reference=1 nblocks=32: 32 | 32 | 1 8 23 | 2 16 14 | 3 29 | 5 27 | 8 24 | 32 | 32
device nsamp=2500000 nchan=12 host_rows=0 reference=1 nblocks=33: 33 | 33 | 1 8 24 | 2 16 15 | 3 30 | 5 28 | 8 25 | 33 | 33
device nsamp=2500000 nchan=12 host_rows=0 reference=1 nblocks=200: 30 170 | 200 | 1 8 64 127 | 2 16 182 | 3 24 173 | 5 40 155 | 8 64 128 | 40 160 | 200
device nsamp=2500000 nchan=12 host_rows=0 reference=1 nblocks=1100: 30 240 830 | 1100 | 1 8 64 512 515 | 2 16 128 954 | 3 24 192 881 | 5 40 320 735 | 8 64 512 516 | 40 320 740 | 1100
device nsamp=2500000 nchan=12 host_rows=0 reference=1 nblocks=30000: 30 240 1920 15360 12450 | 30000 | 1 8 64 512 4096 25319 | 2 16 128 1024 8192 20638 | 3 24 192 1536 12288 15957 | 5 40 320 2560 27075 | 8 64 512 4096 25320 | 40 320 2560 27080 | 30000
device nsamp=2500000 nchan=12 host_rows=0 reference=1 nblocks=1000000: 30 240 1920 15360 122880 859570 | 1000000 | 1 8 64 512 4096 32768 262144 700407 | 2 16 128 1024 8192 65536 524288 400814 | 3 24 192 1536 12288 98304 887653 | 5 40 320 2560 20480 163840 812755 | 8 64 512 4096 32768 262144 700408 | 40 320 2560 20480 163840 812760 | 1000000
device nsamp=2500000 nchan=12 host_rows=1 reference=0 nblocks=1: 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1
device nsamp=2500000 nchan=12 host_rows=1 reference=0 nblocks=31: 31 | 31 | 1 8 22 | 2 16 13 | 3 28 | 5 26 | 8 23 | 31 | 31
device nsamp=2500000 nchan=12 host_rows=1 reference=0 nblocks=32: 32 | 32 | 1 8 23 | 2 16 14 | 3 29 | 5 27 | 8 24 | 32 | 32
device nsamp=2500000 nchan=12 host_rows=1 reference=0 nblocks=33: 33 | 33 | 1 8 24 | 2 16 15 | 3 30 | 5 28 | 8 25 | 33 | 33
device nsamp=2500000 nchan=12 host_rows=1 reference=0 nblocks=200: 71 129 | 200 | 1 8 64 127 | 2 16 182 | 3 24 173 | 5 40 155 | 8 64 128 | 40 160 | 200
device nsamp=2500000 nchan=12 host_rows=1 reference=0 nblocks=1100: 71 568 461 | 1100 | 1 8 64 512 515 | 2 16 128 954 | 3 24 192 881 | 5 40 320 735 | 8 64 512 516 | 40 320 740 | 1100
device nsamp=2500000 nchan=12 host_rows=1 reference=0 nblocks=30000: 71 568 4544 24817 | 30000 | 1 8 64 512 4096 25319 | 2 16 128 1024 8192 20638 | 3 24 192 1536 12288 15957 | 5 40 320 2560 27075 | 8 64 512 4096 25320 | 40 320 2560 27080 | 30000
device nsamp=2500000 nchan=12 host_rows=1 reference=0 nblocks=1000000: 71 568 4544 36352 290816 667649 | 1000000 | 1 8 64 512 4096 32768 262144 700407 | 2 16 128 1024 8192 65536 524288 400814 | 3 24 192 1536 12288 98304 887653 | 5 40 320 2560 20480 163840 812755 | 8 64 512 4096 32768 262144 700408 | 40 320 2560 20480 163840 812760 | 1000000
device nsamp=2500000 nchan=12 host_rows=1 reference=1 nblocks=1: 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1
device nsamp=2500000 nchan=12 host_rows=1 reference=1 nblocks=31: 31 | 31 | 1 8 22 | 2 16 13 | 3 28 | 5 26 | 8 23 | 31 | 31
device nsamp=2500000 nchan=12 host_rows=1 reference=1 nblocks=32: 32 | 32 | 1 8 23 | 2 16 14 | 3 29 | 5 27 | 8 24 | 32 | 32
device nsamp=2500000 nchan=12 host_rows=1 reference=1 nblocks=33: 33 | 33 | 1 8 24 | 2 16 15 | 3 30 | 5 28 | 8 25 | 33 | 33
device nsamp=2500000 nchan=12 host_rows=1 reference=1 nblocks=200: 71 129 | 200 | 1 8 64 127 | 2 16 182 | 3 24 173 | 5 40 155 | 8 64 128 | 40 160 | 200
device nsamp=2500000 nchan=12 host_rows=1 reference=1 nblocks=1100: 71 568 461 | 1100 | 1 8 64 512 515 | 2 16 128 954 | 3 24 192 881 | 5 40 320 735 | 8 64 512 516 | 40 320 740 | 1100
device nsamp=2500000 nchan=12 host_rows=1 reference=1 nblocks=30000: 71 568 4544 24817 | 30000 | 1 8 64 512 4096 25319 | 2 16 128 1024 8192 20638 | 3 24 192 1536 12288 15957 | 5 40 320 2560 27075 | 8 64 512 4096 25320 | 40 320 2560 27080 | 30000
device nsamp=2500000 nchan=12 host_rows=1 reference=1 nblocks=1000000: 71 568 4544 36352 290816 667649 | 1000000 | 1 8 64 512 4096 32768 262144 700407 | 2 16 128 1024 8192 65536 524288 400814 | 3 24 192 1536 12288 98304 887653 | 5 40 320 2560 20480 163840 812755 | 8 64 512 4096 32768 262144 700408 | 40 320 2560 20480 163840 812760 | 1000000
device nsamp=2500000 nchan=16 host_rows=0 reference=0 nblocks=1: 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1
device nsamp=2500000 nchan=16 host_rows=0 reference=0 nblocks=31: 31 | 31 | 1 8 22 | 2 16 13 | 3 28 | 5 26 | 8 23 | 31 | 31
device nsamp=2500000 nchan=16 host_rows=0 reference=0 nblocks=32: 32 | 32 | 1 8 23 | 2 16 14 | 3 29 | 5 27 | 8 24 | 32 | 32
device nsamp=2500000 nchan=16 host_rows=0 reference=0 nblocks=33: 33 | 33 | 1 8 24 | 2 16 15 | 3 30 | 5 28 | 8 25 | 33 | 33
device nsamp=2500000 nchan=16 host_rows=0 reference=0 nblocks=200: 200 | 200 | 1 8 64 127 | 2 16 182 | 3 24 173 | 5 40 155 | 8 64 128 | 40 160 | 200
device nsamp=2500000 nchan=16 host_rows=0 reference=0 nblocks=1100: 1100 | 1100 | 1 8 64 512 515 | 2 16 128 954 | 3 24 192 881 | 5 40 320 735 | 8 64 512 516 | 40 320 740 | 1100
device nsamp=2500000 nchan=16 host_rows=0 reference=0 nblocks=30000: 30000 | 30000 | 1 8 64 512 4096 25319 | 2 16 128 1024 8192 20638 | 3 24 192 1536 12288 15957 | 5 40 320 2560 27075 | 8 64 512 4096 25320 | 40 320 2560 27080 | 30000
device nsamp=2500000 nchan=16 host_rows=0 reference=0 nblocks=1000000: 1000000 | 1000000 | 1 8 64 512 4096 32768 262144 700407 | 2 16 128 1024 8192 65536 524288 400814 | 3 24 192 1536 12288 98304 887653 | 5 40 320 2560 20480 163840 812755 | 8 64 512 4096 32768 262144 700408 | 40 320 2560 20480 163840 812760 | 1000000
device nsamp=2500000 nchan=16 host_rows=0 reference=1 nblocks=1: 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1
device nsamp=2500000 nchan=16 host_rows=0 reference=1 nblocks=31: 31 | 31 | 1 8 22 | 2 16 13 | 3 28 | 5 26 | 8 23 | 31 | 31
device nsamp=2500000 nchan=16 host_rows=0 reference=1 nblocks=32: 32 | 32 | 1 8 23 | 2 16 14 | 3 29 | 5 27 | 8 24 | 32 | 32
device nsamp=2500000 nchan=16 host_rows=0 reference=1 nblocks=33: 33 | 33 | 1 8 24 | 2 16 15 | 3 30 | 5 28 | 8 25 | 33 | 33
device nsamp=2500000 nchan=16 host_rows=0 reference=1 nblocks=200: 23 177 | 200 | 1 8 64 127 | 2 16 182 | 3 24 173 | 5 40 155 | 8 64 128 | 40 160 | 200
device nsamp=2500000 nchan=16 host_rows=0 reference=1 nblocks=1100: 23 184 893 | 1100 | 1 8 64 512 515 | 2 16 128 954 | 3 24 192 881 | 5 40 320 735 | 8 64 512 516 | 40 320 740 | 1100
device nsamp=2500000 nchan=16 host_rows=0 reference=1 nblocks=30000: 23 184 1472 11776 16545 | 30000 | 1 8 64 512 4096 25319 | 2 16 128 1024 8192 20638 | 3 24 192 1536 12288 15957 | 5 40 320 2560 27075 | 8 64 512 4096 25320 | 40 320 2560 27080 | 30000
device nsamp=2500000 nchan=16 host_rows=0 reference=1 nblocks=1000000: 23 184 1472 11776 94208 892337 | 1000000 | 1 8 64 512 4096 32768 262144 700407 | 2 16 128 1024 8192 65536 524288 400814 | 3 24 192 1536 12288 98304 887653 | 5 40 320 2560 20480 163840 812755 | 8 64 512 4096 32768 262144 700408 | 40 320 2560 20480 163840 812760 | 1000000
device nsamp=2500000 nchan=16 host_rows=1 reference=0 nblocks=1: 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1
device nsamp=2500000 nchan=16 host_rows=1 reference=0 nblocks=31: 31 | 31 | 1 8 22 | 2 16 13 | 3 28 | 5 26 | 8 23 | 31 | 31
device nsamp=2500000 nchan=16 host_rows=1 reference=0 nblocks=32: 32 | 32 | 1 8 23 | 2 16 14 | 3 29 | 5 27 | 8 24 | 32 | 32
device nsamp=2500000 nchan=16 host_rows=1 reference=0 nblocks=33: 33 | 33 | 1 8 24 | 2 16 15 | 3 30 | 5 28 | 8 25 | 33 | 33
device nsamp=2500000 nchan=16 host_rows=1 reference=0 nblocks=200: 53 147 | 200 | 1 8 64 127 | 2 16 182 | 3 24 173 | 5 40 155 | 8 64 128 | 40 160 | 200
device nsamp=2500000 nchan=16 host_rows=1 reference=0 nblocks=1100: 53 424 623 | 1100 | 1 8 64 512 515 | 2 16 128 954 | 3 24 192 881 | 5 40 320 735 | 8 64 512 516 | 40 320 740 | 1100
device nsamp=2500000 nchan=16 host_rows=1 reference=0 nblocks=30000: 53 424 3392 26131 | 30000 | 1 8 64 512 4096 25319 | 2 16 128 1024 8192 20638 | 3 24 192 1536 12288 15957 | 5 40 320 2560 27075 | 8 64 512 4096 25320 | 40 320 2560 27080 | 30000
device nsamp=2500000 nchan=16 host_rows=1 reference=0 nblocks=1000000: 53 424 3392 27136 217088 751907 | 1000000 | 1 8 64 512 4096 32768 262144 700407 | 2 16 128 1024 8192 65536 524288 400814 | 3 24 192 1536 12288 98304 887653 | 5 40 320 2560 20480 163840 812755 | 8 64 512 4096 32768 262144 700408 | 40 320 2560 20480 163840 812760 | 1000000
device nsamp=2500000 nchan=16 host_rows=1 reference=1 nblocks=1: 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1 | 1
device nsamp=2500000 nchan=16 host_rows=1 reference=1 nblocks=31: 31 | 31 | 1 8 22 | 2 16 13 | 3 28 | 5 26 | 8 23 | 31 | 31
device nsamp=2500000 nchan=16 host_rows=1 reference=1 nblocks=32: 32 | 32 | 1 8 23 | 2 16 14 | 3 29 | 5 27 | 8 24 | 32 | 32
device nsamp=2500000 nchan=16 host_rows=1 reference=1 nblocks=33: 33 | 33 | 1 8 24 | 2 16 15 | 3 30 | 5 28 | 8 25 | 33 | 33
device nsamp=2500000 nchan=16 host_rows=1 reference=1 nblocks=200: 53 147 | 200 | 1 8 64 127 | 2 16 182 | 3 24 173 | 5 40 155 | 8 64 128 | 40 160 | 200
device nsamp=2500000 nchan=16 host_rows=1 reference=1 nblocks=1100: 53 424 623 | 1100 | 1 8 64 512 515 | 2 16 128 954 | 3 24 192 881 | 5 40 320 735 | 8 64 512 516 | 40 320 740 | 1100
device nsamp=2500000 nchan=16 host_rows=1 reference=1 nblocks=30000: 53 424 3392 26131 | 30000 | 1 8 64 512 4096 25319 | 2 16 128 1024 8192 20638 | 3 24 192 1536 12288 15957 | 5 40 320 2560 27075 | 8 64 512 4096 25320 | 40 320 2560 27080 | 30000
device nsamp=2500000 nchan=16 host_rows=1 reference=1 nblocks=1000000: 53 424 3392 27136 217088 751907 | 1000000 | 1 8 64 512 4096 32768 262144 700407 | 2 16 128 1024 8192 65536 524288 400814 | 3 24 192 1536 12288 98304 887653 | 5 40 320 2560 20480 163840 812755 | 8 64 512 4096 32768 262144 700408 | 40 320 2560 20480 163840 812760 | 1000000
"""


def build(tmp_path, *flags):
    exe = str(tmp_path / "piece_plans")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *flags, "-I" + CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "piece_plans.cpp")], check=True)
    return exe


def test_phase_hand_over_between_pieces(tmp_path):
    """piece_rows (csrc/gpsiq_pieces.h), what the pieces of the staged batch calls hand each other on the host, with no HIP and under
    ASan + UBSan: piece 0 uses the caller's rows as they lie; in a later piece a slot with prn > 0 equal to the row before takes the
    carried phase, a slot whose prn changes at the edge (to another satellite, or to none) keeps its own carr_phase, prn == 0 is
    untouched, and every row but the piece's first is byte-equal to the input -- for 1, 3 and GPSIQ_MAX_CHAN (16) channels, with each
    kind of slot in every position."""
    run = subprocess.run([build(tmp_path, "-fsanitize=address,undefined"), "handover"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    assert run.stdout.splitlines() == ["handover nchan=%d shift=%d: ok" % (n, s) for n in (1, 3, 16) for s in range(4)]


def test_piece_plans_are_the_tables(tmp_path):
    got = subprocess.run([build(tmp_path)], capture_output=True, text=True, check=True, timeout=120).stdout.splitlines()
    want = EXPECTED.splitlines()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
