"""The launch plans of the synthesis kernels (csrc/gpsiq_launch_plan.h) on the CPU: tests/launch_plans.cpp prints plan_synth() for
all nine variants and both sample formats over block lengths either side of a row, a chunk, a generic tile and max_wave_rows; block
counts with no tail, a tail capped at half the blocks and a whole tail; every channel-slot boundary; amplitude bounds either side
of the int16 range with the noise off, on within the range and on past it, the level off and on, GPSIQ_NO_FAST both ways, segm with
and without scratch; and a second grid-shape policy with all four numeric knobs changed.  The table below was not printed by that
header: it is what the launcher printed before the planner was cut out of it -- launch_variant() as it stood at the bottom of
gpsiq_kernels.hip, compiled on its own with every hipLaunchKernelGGL replaced by a line that prints the kernel with its template
arguments, the grid, the block and the integer arguments, and run over the same grid.  The move changed no plan.  The GPU tests
then check the bytes the plans render."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-sdr-gps-sim_amd", "csrc")

# request (variant, bytes per sample component, samples per block, blocks, most active channels, amplitude bound, max |z| of the noise
# or 0 = off, level, scratch given, plain-add allowed, policy 0 = default / 1 = tail_wgs 64, max_wave_rows 128, setup_rows 10,
# drain 2; the swept field last, a run of values where the plan stays) -> the launches: kernel, grid, block, nsamp + shape arguments
EXPECTED = """\
auto ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=0 -> none
auto ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=1 -> synth_generic<2> grid=200 block=256 args=1,1,4096
auto ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=63 -> synth_generic<2> grid=200 block=256 args=63,1,4096
auto ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=64 -> synth_generic<2> grid=200 block=256 args=64,1,4096
auto ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=65 -> synth_generic<2> grid=200 block=256 args=65,1,4096
auto ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=16383 -> synth_generic<2> grid=800 block=256 args=16383,4,4096
auto ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=16384 -> synth_generic<2> grid=800 block=256 args=16384,4,4096
auto ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=16385 -> synth_generic<2> grid=1000 block=256 args=16385,5,4096
auto ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=33333 -> synth_generic<2> grid=1800 block=256 args=33333,9,4096
auto ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=102300 -> synth_generic<2> grid=5000 block=256 args=102300,25,4096
auto ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=260000 -> synth_generic<2> grid=12800 block=256 args=260000,64,4096
auto ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=1000000 -> synth_generic<2> grid=49000 block=256 args=1000000,245,4096
auto ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=2500000 -> synth_generic<2> grid=122200 block=256 args=2500000,611,4096
generic ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=0 -> none
generic ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=1 -> synth_generic<2> grid=200 block=256 args=1,1,4096
generic ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=63 -> synth_generic<2> grid=200 block=256 args=63,1,4096
generic ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=64 -> synth_generic<2> grid=200 block=256 args=64,1,4096
generic ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=65 -> synth_generic<2> grid=200 block=256 args=65,1,4096
generic ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=16383 -> synth_generic<2> grid=800 block=256 args=16383,4,4096
generic ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=16384 -> synth_generic<2> grid=800 block=256 args=16384,4,4096
generic ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=16385 -> synth_generic<2> grid=1000 block=256 args=16385,5,4096
generic ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=33333 -> synth_generic<2> grid=1800 block=256 args=33333,9,4096
generic ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=102300 -> synth_generic<2> grid=5000 block=256 args=102300,25,4096
generic ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=260000 -> synth_generic<2> grid=12800 block=256 args=260000,64,4096
generic ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=1000000 -> synth_generic<2> grid=49000 block=256 args=1000000,245,4096
generic ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=2500000 -> synth_generic<2> grid=122200 block=256 args=2500000,611,4096
rows ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=0 -> none
rows ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=1 -> synth_rows<2> grid=200 block=512 args=1,1
rows ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=63 -> synth_rows<2> grid=200 block=512 args=63,1
rows ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=64 -> synth_rows<2> grid=200 block=512 args=64,1
rows ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=65 -> synth_rows<2> grid=200 block=512 args=65,1
rows ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=16383 -> synth_rows<2> grid=200 block=512 args=16383,1
rows ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=16384 -> synth_rows<2> grid=200 block=512 args=16384,1
rows ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=16385 -> synth_rows<2> grid=400 block=512 args=16385,2
rows ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=33333 -> synth_rows<2> grid=600 block=512 args=33333,3
rows ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=102300 -> synth_rows<2> grid=1400 block=512 args=102300,7
rows ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=260000 -> synth_rows<2> grid=3200 block=512 args=260000,16
rows ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=1000000 -> synth_rows<2> grid=12400 block=512 args=1000000,62
rows ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=2500000 -> synth_rows<2> grid=30600 block=512 args=2500000,153
rowsx ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=0 -> none
rowsx ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=1 -> synth_rowsx<2, 8> grid=200 block=512 args=1,1
rowsx ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=63 -> synth_rowsx<2, 8> grid=200 block=512 args=63,1
rowsx ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=64 -> synth_rowsx<2, 8> grid=200 block=512 args=64,1
rowsx ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=65 -> synth_rowsx<2, 8> grid=200 block=512 args=65,1
rowsx ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=16383 -> synth_rowsx<2, 8> grid=200 block=512 args=16383,1
rowsx ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=16384 -> synth_rowsx<2, 8> grid=200 block=512 args=16384,1
rowsx ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=16385 -> synth_rowsx<2, 8> grid=400 block=512 args=16385,2
rowsx ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=33333 -> synth_rowsx<2, 8> grid=600 block=512 args=33333,3
rowsx ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=102300 -> synth_rowsx<2, 8> grid=1400 block=512 args=102300,7
rowsx ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=260000 -> synth_rowsx<2, 8> grid=3200 block=512 args=260000,16
rowsx ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=1000000 -> synth_rowsx<2, 8> grid=12400 block=512 args=1000000,62
rowsx ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=2500000 -> synth_rowsx<2, 8> grid=30600 block=512 args=2500000,153
tile ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=0 -> none
tile ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=1 -> synth_tile<2, 8, 64, 1, true> grid=200 block=512 args=1,1,64,200,200,1
tile ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=63 -> synth_tile<2, 8, 64, 1, true> grid=200 block=512 args=63,1,64,200,200,1
tile ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=64 -> synth_tile<2, 8, 64, 1, true> grid=200 block=512 args=64,1,64,200,200,1
tile ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=65 -> synth_tile<2, 8, 64, 1, true> grid=200 block=512 args=65,1,64,200,200,1
tile ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=16383 -> synth_tile<2, 8, 64, 1, true> grid=200 block=512 args=16383,1,64,200,200,1
tile ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=16384 -> synth_tile<2, 8, 64, 1, true> grid=200 block=512 args=16384,1,64,200,200,1
tile ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=16385 -> synth_tile<2, 8, 64, 1, true> grid=200 block=512 args=16385,1,64,200,200,1
tile ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=33333 -> synth_tile<2, 8, 64, 1, true> grid=400 block=512 args=33333,2,64,400,200,2
tile ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=102300 -> synth_tile<2, 8, 64, 1, true> grid=800 block=512 args=102300,4,64,800,200,4
tile ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=260000 -> synth_tile<2, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=1000000 -> synth_tile<2, 8, 64, 1, true> grid=6200 block=512 args=1000000,31,64,6200,200,31
tile ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=2500000 -> synth_tile<2, 8, 64, 1, true> grid=15400 block=512 args=2500000,77,64,15400,200,77
seg ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=0 -> none
seg ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=1 -> synth_tile<2, 8, 64, 1, true> grid=200 block=512 args=1,1,64,200,200,1
seg ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=63 -> synth_tile<2, 8, 64, 1, true> grid=200 block=512 args=63,1,64,200,200,1
seg ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=64 -> synth_tile<2, 8, 64, 1, true> grid=200 block=512 args=64,1,64,200,200,1
seg ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=65 -> synth_tile<2, 8, 64, 1, true> grid=200 block=512 args=65,1,64,200,200,1
seg ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=16383 -> synth_tile<2, 8, 64, 1, true> grid=200 block=512 args=16383,1,64,200,200,1
seg ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=16384 -> synth_tile<2, 8, 64, 1, true> grid=200 block=512 args=16384,1,64,200,200,1
seg ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=16385 -> synth_tile<2, 8, 64, 1, true> grid=200 block=512 args=16385,1,64,200,200,1
seg ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=33333 -> synth_tile<2, 8, 64, 1, true> grid=400 block=512 args=33333,2,64,400,200,2
seg ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=102300 -> synth_tile<2, 8, 64, 1, true> grid=800 block=512 args=102300,4,64,800,200,4
seg ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=260000 -> synth_tile<2, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=1000000 -> synth_tile<2, 8, 64, 1, true> grid=4736 block=512 args=1000000,23,85,4209,183,31
seg ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=2500000 -> synth_tile<2, 8, 64, 1, true> grid=6908 block=512 args=2500000,33,148,6369,193,77
segh ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=0 -> none
segh ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=1 -> synth_tile<2, 8, 32, 2, true> grid=200 block=512 args=1,1,32,200,200,1
segh ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=63 -> synth_tile<2, 8, 32, 2, true> grid=200 block=512 args=63,1,32,200,200,1
segh ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=64 -> synth_tile<2, 8, 32, 2, true> grid=200 block=512 args=64,1,32,200,200,1
segh ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=65 -> synth_tile<2, 8, 32, 2, true> grid=200 block=512 args=65,1,32,200,200,1
segh ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=16383 -> synth_tile<2, 8, 32, 2, true> grid=200 block=512 args=16383,1,32,200,200,1
segh ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=16384 -> synth_tile<2, 8, 32, 2, true> grid=200 block=512 args=16384,1,32,200,200,1
segh ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=16385 -> synth_tile<2, 8, 32, 2, true> grid=400 block=512 args=16385,2,32,400,200,2
segh ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=33333 -> synth_tile<2, 8, 32, 2, true> grid=600 block=512 args=33333,3,32,600,200,3
segh ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=102300 -> synth_tile<2, 8, 32, 2, true> grid=1148 block=512 args=102300,5,40,630,126,7
segh ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=260000 -> synth_tile<2, 8, 32, 2, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=1000000 -> synth_tile<2, 8, 32, 2, true> grid=4951 block=512 args=1000000,23,85,4393,191,62
segh ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=2500000 -> synth_tile<2, 8, 32, 2, true> grid=7080 block=512 args=2500000,33,148,6468,196,153
segm ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=0 -> none
segm ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=1 -> sign_masks grid=13 block=256 args=1,200,1,1 ; synth_mask<2, 8> grid=200 block=512 args=1,1,1,1
segm ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=63 -> sign_masks grid=13 block=256 args=63,200,1,1 ; synth_mask<2, 8> grid=200 block=512 args=63,1,1,1
segm ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=64 -> sign_masks grid=13 block=256 args=64,200,1,1 ; synth_mask<2, 8> grid=200 block=512 args=64,1,1,1
segm ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=65 -> sign_masks grid=13 block=256 args=65,200,2,1 ; synth_mask<2, 8> grid=200 block=512 args=65,2,1,1
segm ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=16383 -> sign_masks grid=200 block=256 args=16383,200,256,16 ; synth_mask<2, 8> grid=200 block=512 args=16383,256,1,32
segm ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=16384 -> sign_masks grid=200 block=256 args=16384,200,256,16 ; synth_mask<2, 8> grid=200 block=512 args=16384,256,1,32
segm ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=16385 -> sign_masks grid=213 block=256 args=16385,200,257,17 ; synth_mask<2, 8> grid=200 block=512 args=16385,257,1,33
segm ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=33333 -> sign_masks grid=413 block=256 args=33333,200,521,33 ; synth_mask<2, 8> grid=200 block=512 args=33333,521,1,66
segm ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=102300 -> sign_masks grid=1250 block=256 args=102300,200,1599,100 ; synth_mask<2, 8> grid=200 block=512 args=102300,1599,1,200
segm ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=260000 -> sign_masks grid=3175 block=256 args=260000,200,4063,254 ; synth_mask<2, 8> grid=400 block=512 args=260000,4063,2,254
segm ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=1000000 -> sign_masks grid=12213 block=256 args=1000000,200,15625,977 ; synth_mask<2, 8> grid=1600 block=512 args=1000000,15625,8,245
segm ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=2500000 -> sign_masks grid=30525 block=256 args=2500000,200,39063,2442 ; synth_mask<2, 8> grid=4000 block=512 args=2500000,39063,20,245
segb ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=0 -> none
segb ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=1 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=200 block=512 args=1,1,32,200,200,1
segb ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=63 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=200 block=512 args=63,1,32,200,200,1
segb ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=64 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=200 block=512 args=64,1,32,200,200,1
segb ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=65 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=200 block=512 args=65,1,32,200,200,1
segb ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=16383 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=200 block=512 args=16383,1,32,200,200,1
segb ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=16384 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=200 block=512 args=16384,1,32,200,200,1
segb ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=16385 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=400 block=512 args=16385,2,32,400,200,2
segb ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=33333 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=600 block=512 args=33333,3,32,600,200,3
segb ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=102300 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=1148 block=512 args=102300,5,40,630,126,7
segb ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=260000 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segb ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=1000000 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=4951 block=512 args=1000000,23,85,4393,191,62
segb ss=2 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=2500000 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=7080 block=512 args=2500000,33,148,6468,196,153
auto ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=1 -> synth_generic<2> grid=64 block=256 args=260000,64,4096
auto ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=4130 -> synth_generic<2> grid=264320 block=256 args=260000,64,4096
generic ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=1 -> synth_generic<2> grid=64 block=256 args=260000,64,4096
generic ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=4130 -> synth_generic<2> grid=264320 block=256 args=260000,64,4096
rows ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=1 -> synth_rows<2> grid=16 block=512 args=260000,16
rows ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=4130 -> synth_rows<2> grid=66080 block=512 args=260000,16
rowsx ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=1 -> synth_rowsx<2, 8> grid=16 block=512 args=260000,16
rowsx ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=4130 -> synth_rowsx<2, 8> grid=66080 block=512 args=260000,16
tile ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=1 -> synth_tile<2, 8, 64, 1, true> grid=8 block=512 args=260000,8,64,8,1,8
tile ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=2 -> synth_tile<2, 8, 64, 1, true> grid=16 block=512 args=260000,8,64,16,2,8
tile ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=3 -> synth_tile<2, 8, 64, 1, true> grid=24 block=512 args=260000,8,64,24,3,8
tile ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=7 -> synth_tile<2, 8, 64, 1, true> grid=56 block=512 args=260000,8,64,56,7,8
tile ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=26 -> synth_tile<2, 8, 64, 1, true> grid=208 block=512 args=260000,8,64,208,26,8
tile ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=200 -> synth_tile<2, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=2000 -> synth_tile<2, 8, 64, 1, true> grid=16000 block=512 args=260000,8,64,16000,2000,8
tile ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=4130 -> synth_tile<2, 8, 64, 1, true> grid=33040 block=512 args=260000,8,64,33040,4130,8
tile ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=1 -> synth_tile<2, 8, 64, 1, true> grid=77 block=512 args=2500000,77,64,77,1,77
tile ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=2 -> synth_tile<2, 8, 64, 1, true> grid=154 block=512 args=2500000,77,64,154,2,77
tile ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=3 -> synth_tile<2, 8, 64, 1, true> grid=231 block=512 args=2500000,77,64,231,3,77
tile ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=7 -> synth_tile<2, 8, 64, 1, true> grid=539 block=512 args=2500000,77,64,539,7,77
tile ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=26 -> synth_tile<2, 8, 64, 1, true> grid=2002 block=512 args=2500000,77,64,2002,26,77
tile ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=200 -> synth_tile<2, 8, 64, 1, true> grid=15400 block=512 args=2500000,77,64,15400,200,77
tile ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=2000 -> synth_tile<2, 8, 64, 1, true> grid=154000 block=512 args=2500000,77,64,154000,2000,77
tile ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=4130 -> synth_tile<2, 8, 64, 1, true> grid=318010 block=512 args=2500000,77,64,318010,4130,77
seg ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=1 -> synth_tile<2, 8, 64, 1, true> grid=8 block=512 args=260000,8,64,8,1,8
seg ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=2 -> synth_tile<2, 8, 64, 1, true> grid=16 block=512 args=260000,8,64,16,2,8
seg ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=3 -> synth_tile<2, 8, 64, 1, true> grid=24 block=512 args=260000,8,64,24,3,8
seg ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=7 -> synth_tile<2, 8, 64, 1, true> grid=56 block=512 args=260000,8,64,56,7,8
seg ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=26 -> synth_tile<2, 8, 64, 1, true> grid=208 block=512 args=260000,8,64,208,26,8
seg ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=200 -> synth_tile<2, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=2000 -> synth_tile<2, 8, 64, 1, true> grid=8256 block=512 args=260000,4,127,7744,1936,8
seg ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=4130 -> synth_tile<2, 8, 64, 1, true> grid=8644 block=512 args=260000,2,254,8132,4066,8
seg ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=1 -> synth_tile<2, 8, 64, 1, true> grid=77 block=512 args=2500000,77,64,77,1,77
seg ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=2 -> synth_tile<2, 8, 64, 1, true> grid=154 block=512 args=2500000,77,64,154,2,77
seg ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=3 -> synth_tile<2, 8, 64, 1, true> grid=231 block=512 args=2500000,77,64,231,3,77
seg ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=7 -> synth_tile<2, 8, 64, 1, true> grid=527 block=512 args=2500000,74,66,296,4,77
seg ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=26 -> synth_tile<2, 8, 64, 1, true> grid=1945 block=512 args=2500000,74,66,1406,19,77
seg ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=200 -> synth_tile<2, 8, 64, 1, true> grid=6908 block=512 args=2500000,33,148,6369,193,77
seg ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=2000 -> synth_tile<2, 8, 64, 1, true> grid=22462 block=512 args=2500000,11,444,21923,1993,77
seg ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=4130 -> synth_tile<2, 8, 64, 1, true> grid=45892 block=512 args=2500000,11,444,45353,4123,77
segh ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=1 -> synth_tile<2, 8, 32, 2, true> grid=16 block=512 args=260000,16,32,16,1,16
segh ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=2 -> synth_tile<2, 8, 32, 2, true> grid=32 block=512 args=260000,16,32,32,2,16
segh ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=3 -> synth_tile<2, 8, 32, 2, true> grid=48 block=512 args=260000,16,32,48,3,16
segh ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=7 -> synth_tile<2, 8, 32, 2, true> grid=112 block=512 args=260000,16,32,112,7,16
segh ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=26 -> synth_tile<2, 8, 32, 2, true> grid=416 block=512 args=260000,16,32,416,26,16
segh ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=200 -> synth_tile<2, 8, 32, 2, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=2000 -> synth_tile<2, 8, 32, 2, true> grid=8384 block=512 args=260000,4,127,7872,1968,16
segh ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=4130 -> synth_tile<2, 8, 32, 2, true> grid=8708 block=512 args=260000,2,254,8196,4098,16
segh ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=1 -> synth_tile<2, 8, 32, 2, true> grid=153 block=512 args=2500000,153,32,153,1,153
segh ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=2 -> synth_tile<2, 8, 32, 2, true> grid=306 block=512 args=2500000,153,32,306,2,153
segh ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=3 -> synth_tile<2, 8, 32, 2, true> grid=459 block=512 args=2500000,153,32,459,3,153
segh ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=7 -> synth_tile<2, 8, 32, 2, true> grid=1051 block=512 args=2500000,148,33,592,4,153
segh ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=26 -> synth_tile<2, 8, 32, 2, true> grid=2680 block=512 args=2500000,94,52,2068,22,153
segh ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=200 -> synth_tile<2, 8, 32, 2, true> grid=7080 block=512 args=2500000,33,148,6468,196,153
segh ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=2000 -> synth_tile<2, 8, 32, 2, true> grid=22568 block=512 args=2500000,11,444,21956,1996,153
segh ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=4130 -> synth_tile<2, 8, 32, 2, true> grid=45998 block=512 args=2500000,11,444,45386,4126,153
segm ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=1 -> sign_masks grid=16 block=256 args=260000,1,4063,254 ; synth_mask<2, 8> grid=2 block=512 args=260000,4063,2,254
segm ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=2 -> sign_masks grid=32 block=256 args=260000,2,4063,254 ; synth_mask<2, 8> grid=4 block=512 args=260000,4063,2,254
segm ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=3 -> sign_masks grid=48 block=256 args=260000,3,4063,254 ; synth_mask<2, 8> grid=6 block=512 args=260000,4063,2,254
segm ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=7 -> sign_masks grid=112 block=256 args=260000,7,4063,254 ; synth_mask<2, 8> grid=14 block=512 args=260000,4063,2,254
segm ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=26 -> sign_masks grid=413 block=256 args=260000,26,4063,254 ; synth_mask<2, 8> grid=52 block=512 args=260000,4063,2,254
segm ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=200 -> sign_masks grid=3175 block=256 args=260000,200,4063,254 ; synth_mask<2, 8> grid=400 block=512 args=260000,4063,2,254
segm ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=2000 -> sign_masks grid=31750 block=256 args=260000,2000,4063,254 ; synth_mask<2, 8> grid=4000 block=512 args=260000,4063,2,254
segm ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=4130 -> sign_masks grid=65564 block=256 args=260000,4130,4063,254 ; synth_mask<2, 8> grid=8260 block=512 args=260000,4063,2,254
segm ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=1 -> sign_masks grid=153 block=256 args=2500000,1,39063,2442 ; synth_mask<2, 8> grid=20 block=512 args=2500000,39063,20,245
segm ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=2 -> sign_masks grid=306 block=256 args=2500000,2,39063,2442 ; synth_mask<2, 8> grid=40 block=512 args=2500000,39063,20,245
segm ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=3 -> sign_masks grid=458 block=256 args=2500000,3,39063,2442 ; synth_mask<2, 8> grid=60 block=512 args=2500000,39063,20,245
segm ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=7 -> sign_masks grid=1069 block=256 args=2500000,7,39063,2442 ; synth_mask<2, 8> grid=140 block=512 args=2500000,39063,20,245
segm ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=26 -> sign_masks grid=3969 block=256 args=2500000,26,39063,2442 ; synth_mask<2, 8> grid=520 block=512 args=2500000,39063,20,245
segm ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=200 -> sign_masks grid=30525 block=256 args=2500000,200,39063,2442 ; synth_mask<2, 8> grid=4000 block=512 args=2500000,39063,20,245
segm ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=2000 -> sign_masks grid=305250 block=256 args=2500000,2000,39063,2442 ; synth_mask<2, 8> grid=40000 block=512 args=2500000,39063,20,245
segm ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=4130 -> sign_masks grid=630342 block=256 args=2500000,4130,39063,2442 ; synth_mask<2, 8> grid=82600 block=512 args=2500000,39063,20,245
segb ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=1 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=16 block=512 args=260000,16,32,16,1,16
segb ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=2 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=32 block=512 args=260000,16,32,32,2,16
segb ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=3 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=48 block=512 args=260000,16,32,48,3,16
segb ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=7 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=112 block=512 args=260000,16,32,112,7,16
segb ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=26 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=416 block=512 args=260000,16,32,416,26,16
segb ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=200 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segb ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=2000 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=8384 block=512 args=260000,4,127,7872,1968,16
segb ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=4130 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=8708 block=512 args=260000,2,254,8196,4098,16
segb ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=1 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=153 block=512 args=2500000,153,32,153,1,153
segb ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=2 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=306 block=512 args=2500000,153,32,306,2,153
segb ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=3 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=459 block=512 args=2500000,153,32,459,3,153
segb ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=7 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=1051 block=512 args=2500000,148,33,592,4,153
segb ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=26 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=2680 block=512 args=2500000,94,52,2068,22,153
segb ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=200 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=7080 block=512 args=2500000,33,148,6468,196,153
segb ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=2000 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=22568 block=512 args=2500000,11,444,21956,1996,153
segb ss=2 n=2500000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=4130 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=45998 block=512 args=2500000,11,444,45386,4126,153
seg ss=2 n=260000 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 nb=0 -> none
auto ss=1 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=65 -> synth_generic<1> grid=200 block=256 args=65,1,4096
auto ss=1 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=260000 -> synth_generic<1> grid=12800 block=256 args=260000,64,4096
generic ss=1 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=65 -> synth_generic<1> grid=200 block=256 args=65,1,4096
generic ss=1 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=260000 -> synth_generic<1> grid=12800 block=256 args=260000,64,4096
rows ss=1 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=65 -> synth_rows<1> grid=200 block=512 args=65,1
rows ss=1 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=260000 -> synth_rows<1> grid=3200 block=512 args=260000,16
rowsx ss=1 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=65 -> synth_rowsx<1, 8> grid=200 block=512 args=65,1
rowsx ss=1 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=260000 -> synth_rowsx<1, 8> grid=3200 block=512 args=260000,16
tile ss=1 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=65 -> synth_tile<1, 8, 64, 1, true> grid=200 block=512 args=65,1,64,200,200,1
tile ss=1 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=260000 -> synth_tile<1, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=1 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=65 -> synth_tile<1, 8, 64, 1, true> grid=200 block=512 args=65,1,64,200,200,1
seg ss=1 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=260000 -> synth_tile<1, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
segh ss=1 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=65 -> synth_tile<1, 8, 32, 2, true> grid=200 block=512 args=65,1,32,200,200,1
segh ss=1 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=260000 -> synth_tile<1, 8, 32, 2, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segm ss=1 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=65 -> sign_masks grid=13 block=256 args=65,200,2,1 ; synth_mask<1, 8> grid=200 block=512 args=65,2,1,1
segm ss=1 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=260000 -> sign_masks grid=3175 block=256 args=260000,200,4063,254 ; synth_mask<1, 8> grid=400 block=512 args=260000,4063,2,254
segb ss=1 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=65 -> synth_tile<1, 8, 32, 1, true, 8, true> grid=200 block=512 args=65,1,32,200,200,1
segb ss=1 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 n=260000 -> synth_tile<1, 8, 32, 1, true, 8, true> grid=2192 block=512 args=260000,10,51,1680,168,16
rowsx ss=2 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=1,4 -> synth_rowsx<2, 4> grid=3200 block=512 args=260000,16
rowsx ss=2 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=5,8 -> synth_rowsx<2, 8> grid=3200 block=512 args=260000,16
rowsx ss=2 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=9,12,13,16 -> synth_rowsx<2, 16> grid=3200 block=512 args=260000,16
rowsx ss=1 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=1,4 -> synth_rowsx<1, 4> grid=3200 block=512 args=260000,16
rowsx ss=1 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=5,8 -> synth_rowsx<1, 8> grid=3200 block=512 args=260000,16
rowsx ss=1 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=9,12,13,16 -> synth_rowsx<1, 16> grid=3200 block=512 args=260000,16
tile ss=2 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=1,4 -> synth_tile<2, 4, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=2 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=5,8 -> synth_tile<2, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=2 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=9,12 -> synth_tile<2, 12, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=2 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=13,16 -> synth_tile<2, 16, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=1 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=1,4 -> synth_tile<1, 4, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=1 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=5,8 -> synth_tile<1, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=1 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=9,12 -> synth_tile<1, 12, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=1 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=13,16 -> synth_tile<1, 16, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=2 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=1,4 -> synth_tile<2, 4, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=2 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=5,8 -> synth_tile<2, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=2 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=9,12 -> synth_tile<2, 12, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=2 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=13,16 -> synth_tile<2, 16, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=1 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=1,4 -> synth_tile<1, 4, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=1 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=5,8 -> synth_tile<1, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=1 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=9,12 -> synth_tile<1, 12, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=1 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=13,16 -> synth_tile<1, 16, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
segh ss=2 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=1,4 -> synth_tile<2, 4, 32, 2, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=2 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=5,8 -> synth_tile<2, 8, 32, 2, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=2 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=9,12 -> synth_tile<2, 12, 32, 2, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=2 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=13,16 -> synth_tile<2, 16, 32, 2, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=1 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=1,4 -> synth_tile<1, 4, 32, 2, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=1 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=5,8 -> synth_tile<1, 8, 32, 2, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=1 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=9,12 -> synth_tile<1, 12, 32, 2, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=1 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=13,16 -> synth_tile<1, 16, 32, 2, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segm ss=2 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=1,4 -> sign_masks grid=3175 block=256 args=260000,200,4063,254 ; synth_mask<2, 4> grid=400 block=512 args=260000,4063,2,254
segm ss=2 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=5,8 -> sign_masks grid=3175 block=256 args=260000,200,4063,254 ; synth_mask<2, 8> grid=400 block=512 args=260000,4063,2,254
segm ss=2 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=9,12 -> sign_masks grid=3175 block=256 args=260000,200,4063,254 ; synth_mask<2, 12> grid=400 block=512 args=260000,4063,2,254
segm ss=2 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=13,16 -> sign_masks grid=3175 block=256 args=260000,200,4063,254 ; synth_mask<2, 16> grid=400 block=512 args=260000,4063,2,254
segm ss=1 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=1,4 -> sign_masks grid=3175 block=256 args=260000,200,4063,254 ; synth_mask<1, 4> grid=400 block=512 args=260000,4063,2,254
segm ss=1 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=5,8 -> sign_masks grid=3175 block=256 args=260000,200,4063,254 ; synth_mask<1, 8> grid=400 block=512 args=260000,4063,2,254
segm ss=1 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=9,12 -> sign_masks grid=3175 block=256 args=260000,200,4063,254 ; synth_mask<1, 12> grid=400 block=512 args=260000,4063,2,254
segm ss=1 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=13,16 -> sign_masks grid=3175 block=256 args=260000,200,4063,254 ; synth_mask<1, 16> grid=400 block=512 args=260000,4063,2,254
segb ss=2 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=1,4 -> synth_tile<2, 4, 64, 1, true, 8, true> grid=1600 block=512 args=260000,8,64,1600,200,8
segb ss=2 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=5,8 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segb ss=2 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=9,12 -> synth_tile<2, 12, 16, 1, true, 8, true> grid=2352 block=512 args=260000,10,51,1840,184,32
segb ss=2 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=13,16 -> synth_tile<2, 16, 16, 1, true, 8, true> grid=2352 block=512 args=260000,10,51,1840,184,32
segb ss=1 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=1,4 -> synth_tile<1, 4, 64, 1, true, 8, true> grid=1600 block=512 args=260000,8,64,1600,200,8
segb ss=1 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=5,8 -> synth_tile<1, 8, 32, 1, true, 8, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segb ss=1 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=9,12 -> synth_tile<1, 12, 16, 1, true, 8, true> grid=2352 block=512 args=260000,10,51,1840,184,32
segb ss=1 n=260000 nb=200 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 act=13,16 -> synth_tile<1, 16, 16, 1, true, 8, true> grid=2352 block=512 args=260000,10,51,1840,184,32
tile ss=2 n=260000 nb=200 act=8 z=0 lv=0 scr=1 fast=1 pol=0 amp=0,32667,32767 -> synth_tile<2, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=2 n=260000 nb=200 act=8 z=0 lv=0 scr=1 fast=1 pol=0 amp=32768 -> synth_tile<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=2 n=260000 nb=200 act=8 z=0 lv=0 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=2 n=260000 nb=200 act=8 z=0 lv=1 scr=1 fast=1 pol=0 amp=0,32667,32767 -> synth_tile_level<2, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=2 n=260000 nb=200 act=8 z=0 lv=1 scr=1 fast=1 pol=0 amp=32768 -> synth_tile_level<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=2 n=260000 nb=200 act=8 z=0 lv=1 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_level<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=2 n=260000 nb=200 act=8 z=100 lv=0 scr=1 fast=1 pol=0 amp=0,32667 -> synth_tile_noise<2, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=2 n=260000 nb=200 act=8 z=100 lv=0 scr=1 fast=1 pol=0 amp=32767,32768 -> synth_tile_noise<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=2 n=260000 nb=200 act=8 z=100 lv=0 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_noise<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=2 n=260000 nb=200 act=8 z=100 lv=1 scr=1 fast=1 pol=0 amp=0,32667,32767 -> synth_tile_level<2, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=2 n=260000 nb=200 act=8 z=100 lv=1 scr=1 fast=1 pol=0 amp=32768 -> synth_tile_level<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=2 n=260000 nb=200 act=8 z=100 lv=1 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_level<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=2 n=260000 nb=200 act=8 z=40000 lv=0 scr=1 fast=1 pol=0 amp=0,32667,32767,32768 -> synth_tile_noise<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=2 n=260000 nb=200 act=8 z=40000 lv=0 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_noise<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=2 n=260000 nb=200 act=8 z=40000 lv=1 scr=1 fast=1 pol=0 amp=0,32667,32767 -> synth_tile_level<2, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=2 n=260000 nb=200 act=8 z=40000 lv=1 scr=1 fast=1 pol=0 amp=32768 -> synth_tile_level<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=2 n=260000 nb=200 act=8 z=40000 lv=1 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_level<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=1 n=260000 nb=200 act=8 z=0 lv=0 scr=1 fast=1 pol=0 amp=0,32667,32767,32768 -> synth_tile<1, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=1 n=260000 nb=200 act=8 z=0 lv=0 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile<1, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=1 n=260000 nb=200 act=8 z=0 lv=1 scr=1 fast=1 pol=0 amp=0,32667,32767 -> synth_tile_level<1, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=1 n=260000 nb=200 act=8 z=0 lv=1 scr=1 fast=1 pol=0 amp=32768 -> synth_tile_level<1, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=1 n=260000 nb=200 act=8 z=0 lv=1 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_level<1, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=1 n=260000 nb=200 act=8 z=100 lv=0 scr=1 fast=1 pol=0 amp=0,32667,32767,32768 -> synth_tile_noise<1, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=1 n=260000 nb=200 act=8 z=100 lv=0 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_noise<1, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=1 n=260000 nb=200 act=8 z=100 lv=1 scr=1 fast=1 pol=0 amp=0,32667,32767 -> synth_tile_level<1, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=1 n=260000 nb=200 act=8 z=100 lv=1 scr=1 fast=1 pol=0 amp=32768 -> synth_tile_level<1, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=1 n=260000 nb=200 act=8 z=100 lv=1 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_level<1, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=1 n=260000 nb=200 act=8 z=40000 lv=0 scr=1 fast=1 pol=0 amp=0,32667,32767,32768 -> synth_tile_noise<1, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=1 n=260000 nb=200 act=8 z=40000 lv=0 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_noise<1, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=1 n=260000 nb=200 act=8 z=40000 lv=1 scr=1 fast=1 pol=0 amp=0,32667,32767 -> synth_tile_level<1, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=1 n=260000 nb=200 act=8 z=40000 lv=1 scr=1 fast=1 pol=0 amp=32768 -> synth_tile_level<1, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=1 n=260000 nb=200 act=8 z=40000 lv=1 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_level<1, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=2 n=260000 nb=200 act=8 z=0 lv=0 scr=1 fast=1 pol=0 amp=0,32667,32767 -> synth_tile<2, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=2 n=260000 nb=200 act=8 z=0 lv=0 scr=1 fast=1 pol=0 amp=32768 -> synth_tile<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=2 n=260000 nb=200 act=8 z=0 lv=0 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=2 n=260000 nb=200 act=8 z=0 lv=1 scr=1 fast=1 pol=0 amp=0,32667,32767 -> synth_tile_level<2, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=2 n=260000 nb=200 act=8 z=0 lv=1 scr=1 fast=1 pol=0 amp=32768 -> synth_tile_level<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=2 n=260000 nb=200 act=8 z=0 lv=1 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_level<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=2 n=260000 nb=200 act=8 z=100 lv=0 scr=1 fast=1 pol=0 amp=0,32667 -> synth_tile_noise<2, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=2 n=260000 nb=200 act=8 z=100 lv=0 scr=1 fast=1 pol=0 amp=32767,32768 -> synth_tile_noise<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=2 n=260000 nb=200 act=8 z=100 lv=0 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_noise<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=2 n=260000 nb=200 act=8 z=100 lv=1 scr=1 fast=1 pol=0 amp=0,32667,32767 -> synth_tile_level<2, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=2 n=260000 nb=200 act=8 z=100 lv=1 scr=1 fast=1 pol=0 amp=32768 -> synth_tile_level<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=2 n=260000 nb=200 act=8 z=100 lv=1 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_level<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=2 n=260000 nb=200 act=8 z=40000 lv=0 scr=1 fast=1 pol=0 amp=0,32667,32767,32768 -> synth_tile_noise<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=2 n=260000 nb=200 act=8 z=40000 lv=0 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_noise<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=2 n=260000 nb=200 act=8 z=40000 lv=1 scr=1 fast=1 pol=0 amp=0,32667,32767 -> synth_tile_level<2, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=2 n=260000 nb=200 act=8 z=40000 lv=1 scr=1 fast=1 pol=0 amp=32768 -> synth_tile_level<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=2 n=260000 nb=200 act=8 z=40000 lv=1 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_level<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=1 n=260000 nb=200 act=8 z=0 lv=0 scr=1 fast=1 pol=0 amp=0,32667,32767,32768 -> synth_tile<1, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=1 n=260000 nb=200 act=8 z=0 lv=0 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile<1, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=1 n=260000 nb=200 act=8 z=0 lv=1 scr=1 fast=1 pol=0 amp=0,32667,32767 -> synth_tile_level<1, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=1 n=260000 nb=200 act=8 z=0 lv=1 scr=1 fast=1 pol=0 amp=32768 -> synth_tile_level<1, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=1 n=260000 nb=200 act=8 z=0 lv=1 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_level<1, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=1 n=260000 nb=200 act=8 z=100 lv=0 scr=1 fast=1 pol=0 amp=0,32667,32767,32768 -> synth_tile_noise<1, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=1 n=260000 nb=200 act=8 z=100 lv=0 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_noise<1, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=1 n=260000 nb=200 act=8 z=100 lv=1 scr=1 fast=1 pol=0 amp=0,32667,32767 -> synth_tile_level<1, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=1 n=260000 nb=200 act=8 z=100 lv=1 scr=1 fast=1 pol=0 amp=32768 -> synth_tile_level<1, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=1 n=260000 nb=200 act=8 z=100 lv=1 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_level<1, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=1 n=260000 nb=200 act=8 z=40000 lv=0 scr=1 fast=1 pol=0 amp=0,32667,32767,32768 -> synth_tile_noise<1, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=1 n=260000 nb=200 act=8 z=40000 lv=0 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_noise<1, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=1 n=260000 nb=200 act=8 z=40000 lv=1 scr=1 fast=1 pol=0 amp=0,32667,32767 -> synth_tile_level<1, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=1 n=260000 nb=200 act=8 z=40000 lv=1 scr=1 fast=1 pol=0 amp=32768 -> synth_tile_level<1, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=1 n=260000 nb=200 act=8 z=40000 lv=1 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_level<1, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
segh ss=2 n=260000 nb=200 act=8 z=0 lv=0 scr=1 fast=1 pol=0 amp=0,32667,32767 -> synth_tile<2, 8, 32, 2, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=2 n=260000 nb=200 act=8 z=0 lv=0 scr=1 fast=1 pol=0 amp=32768 -> synth_tile<2, 8, 32, 2, false> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=2 n=260000 nb=200 act=8 z=0 lv=0 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile<2, 8, 32, 2, false> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=2 n=260000 nb=200 act=8 z=0 lv=1 scr=1 fast=1 pol=0 amp=0,32667,32767 -> synth_tile_level<2, 8, 32, 2, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=2 n=260000 nb=200 act=8 z=0 lv=1 scr=1 fast=1 pol=0 amp=32768 -> synth_tile_level<2, 8, 32, 2, false> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=2 n=260000 nb=200 act=8 z=0 lv=1 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_level<2, 8, 32, 2, false> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=2 n=260000 nb=200 act=8 z=100 lv=0 scr=1 fast=1 pol=0 amp=0,32667 -> synth_tile_noise<2, 8, 32, 2, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=2 n=260000 nb=200 act=8 z=100 lv=0 scr=1 fast=1 pol=0 amp=32767,32768 -> synth_tile_noise<2, 8, 32, 2, false> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=2 n=260000 nb=200 act=8 z=100 lv=0 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_noise<2, 8, 32, 2, false> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=2 n=260000 nb=200 act=8 z=100 lv=1 scr=1 fast=1 pol=0 amp=0,32667,32767 -> synth_tile_level<2, 8, 32, 2, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=2 n=260000 nb=200 act=8 z=100 lv=1 scr=1 fast=1 pol=0 amp=32768 -> synth_tile_level<2, 8, 32, 2, false> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=2 n=260000 nb=200 act=8 z=100 lv=1 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_level<2, 8, 32, 2, false> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=2 n=260000 nb=200 act=8 z=40000 lv=0 scr=1 fast=1 pol=0 amp=0,32667,32767,32768 -> synth_tile_noise<2, 8, 32, 2, false> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=2 n=260000 nb=200 act=8 z=40000 lv=0 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_noise<2, 8, 32, 2, false> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=2 n=260000 nb=200 act=8 z=40000 lv=1 scr=1 fast=1 pol=0 amp=0,32667,32767 -> synth_tile_level<2, 8, 32, 2, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=2 n=260000 nb=200 act=8 z=40000 lv=1 scr=1 fast=1 pol=0 amp=32768 -> synth_tile_level<2, 8, 32, 2, false> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=2 n=260000 nb=200 act=8 z=40000 lv=1 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_level<2, 8, 32, 2, false> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=1 n=260000 nb=200 act=8 z=0 lv=0 scr=1 fast=1 pol=0 amp=0,32667,32767,32768 -> synth_tile<1, 8, 32, 2, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=1 n=260000 nb=200 act=8 z=0 lv=0 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile<1, 8, 32, 2, false> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=1 n=260000 nb=200 act=8 z=0 lv=1 scr=1 fast=1 pol=0 amp=0,32667,32767 -> synth_tile_level<1, 8, 32, 2, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=1 n=260000 nb=200 act=8 z=0 lv=1 scr=1 fast=1 pol=0 amp=32768 -> synth_tile_level<1, 8, 32, 2, false> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=1 n=260000 nb=200 act=8 z=0 lv=1 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_level<1, 8, 32, 2, false> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=1 n=260000 nb=200 act=8 z=100 lv=0 scr=1 fast=1 pol=0 amp=0,32667,32767,32768 -> synth_tile_noise<1, 8, 32, 2, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=1 n=260000 nb=200 act=8 z=100 lv=0 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_noise<1, 8, 32, 2, false> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=1 n=260000 nb=200 act=8 z=100 lv=1 scr=1 fast=1 pol=0 amp=0,32667,32767 -> synth_tile_level<1, 8, 32, 2, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=1 n=260000 nb=200 act=8 z=100 lv=1 scr=1 fast=1 pol=0 amp=32768 -> synth_tile_level<1, 8, 32, 2, false> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=1 n=260000 nb=200 act=8 z=100 lv=1 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_level<1, 8, 32, 2, false> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=1 n=260000 nb=200 act=8 z=40000 lv=0 scr=1 fast=1 pol=0 amp=0,32667,32767,32768 -> synth_tile_noise<1, 8, 32, 2, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=1 n=260000 nb=200 act=8 z=40000 lv=0 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_noise<1, 8, 32, 2, false> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=1 n=260000 nb=200 act=8 z=40000 lv=1 scr=1 fast=1 pol=0 amp=0,32667,32767 -> synth_tile_level<1, 8, 32, 2, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=1 n=260000 nb=200 act=8 z=40000 lv=1 scr=1 fast=1 pol=0 amp=32768 -> synth_tile_level<1, 8, 32, 2, false> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=1 n=260000 nb=200 act=8 z=40000 lv=1 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile_level<1, 8, 32, 2, false> grid=2192 block=512 args=260000,10,51,1680,168,16
segm ss=2 n=260000 nb=200 act=8 z=0 lv=0 scr=1 fast=1 pol=0 amp=0,32667,32767 -> sign_masks grid=3175 block=256 args=260000,200,4063,254 ; synth_mask<2, 8> grid=400 block=512 args=260000,4063,2,254
segm ss=2 n=260000 nb=200 act=8 z=0 lv=0 scr=1 fast=1 pol=0 amp=32768 -> synth_tile<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
segm ss=2 n=260000 nb=200 act=8 z=0 lv=0 scr=1 fast=0 pol=0 amp=0,32667,32767 -> sign_masks grid=3175 block=256 args=260000,200,4063,254 ; synth_mask<2, 8> grid=400 block=512 args=260000,4063,2,254
segm ss=2 n=260000 nb=200 act=8 z=0 lv=0 scr=1 fast=0 pol=0 amp=32768 -> synth_tile<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
segm ss=2 n=260000 nb=200 act=8 z=0 lv=0 scr=0 fast=1 pol=0 amp=0,32667,32767 -> synth_tile<2, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
segm ss=2 n=260000 nb=200 act=8 z=0 lv=0 scr=0 fast=1 pol=0 amp=32768 -> synth_tile<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
segm ss=2 n=260000 nb=200 act=8 z=0 lv=0 scr=0 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
segm ss=1 n=260000 nb=200 act=8 z=0 lv=0 scr=1 fast=1 pol=0 amp=0,32667,32767,32768 -> sign_masks grid=3175 block=256 args=260000,200,4063,254 ; synth_mask<1, 8> grid=400 block=512 args=260000,4063,2,254
segm ss=1 n=260000 nb=200 act=8 z=0 lv=0 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> sign_masks grid=3175 block=256 args=260000,200,4063,254 ; synth_mask<1, 8> grid=400 block=512 args=260000,4063,2,254
segm ss=1 n=260000 nb=200 act=8 z=0 lv=0 scr=0 fast=1 pol=0 amp=0,32667,32767,32768 -> synth_tile<1, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
segm ss=1 n=260000 nb=200 act=8 z=0 lv=0 scr=0 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile<1, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
segb ss=2 n=260000 nb=200 act=8 z=0 lv=0 scr=1 fast=1 pol=0 amp=0,32667,32767 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segb ss=2 n=260000 nb=200 act=8 z=0 lv=0 scr=1 fast=1 pol=0 amp=32768 -> synth_tile<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
segb ss=2 n=260000 nb=200 act=8 z=0 lv=0 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile<2, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
segb ss=1 n=260000 nb=200 act=8 z=0 lv=0 scr=1 fast=1 pol=0 amp=0,32667,32767,32768 -> synth_tile<1, 8, 32, 1, true, 8, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segb ss=1 n=260000 nb=200 act=8 z=0 lv=0 scr=1 fast=0 pol=0 amp=0,32667,32767,32768 -> synth_tile<1, 8, 64, 1, false> grid=1600 block=512 args=260000,8,64,1600,200,8
auto ss=2 n=260000 nb=200 act=8 amp=1000 lv=0 scr=1 fast=1 pol=0 z=100 -> invalid
auto ss=2 n=260000 nb=200 act=8 amp=1000 lv=1 scr=1 fast=1 pol=0 z=0,100 -> invalid
generic ss=2 n=260000 nb=200 act=8 amp=1000 lv=0 scr=1 fast=1 pol=0 z=100 -> synth_generic<2> grid=12800 block=256 args=260000,64,4096
generic ss=2 n=260000 nb=200 act=8 amp=1000 lv=1 scr=1 fast=1 pol=0 z=0,100 -> synth_generic<2> grid=12800 block=256 args=260000,64,4096
rows ss=2 n=260000 nb=200 act=8 amp=1000 lv=0 scr=1 fast=1 pol=0 z=100 -> invalid
rows ss=2 n=260000 nb=200 act=8 amp=1000 lv=1 scr=1 fast=1 pol=0 z=0,100 -> invalid
rowsx ss=2 n=260000 nb=200 act=8 amp=1000 lv=0 scr=1 fast=1 pol=0 z=100 -> invalid
rowsx ss=2 n=260000 nb=200 act=8 amp=1000 lv=1 scr=1 fast=1 pol=0 z=0,100 -> invalid
segm ss=2 n=260000 nb=200 act=8 amp=1000 lv=0 scr=1 fast=1 pol=0 z=100 -> invalid
segm ss=2 n=260000 nb=200 act=8 amp=1000 lv=1 scr=1 fast=1 pol=0 z=0,100 -> invalid
segb ss=2 n=260000 nb=200 act=8 amp=1000 lv=0 scr=1 fast=1 pol=0 z=100 -> invalid
segb ss=2 n=260000 nb=200 act=8 amp=1000 lv=1 scr=1 fast=1 pol=0 z=0,100 -> invalid
tile ss=2 n=65 nb=7 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0,1 -> synth_tile<2, 8, 64, 1, true> grid=7 block=512 args=65,1,64,7,7,1
tile ss=2 n=65 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0,1 -> synth_tile<2, 8, 64, 1, true> grid=200 block=512 args=65,1,64,200,200,1
tile ss=2 n=16385 nb=7 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0,1 -> synth_tile<2, 8, 64, 1, true> grid=7 block=512 args=16385,1,64,7,7,1
tile ss=2 n=16385 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0,1 -> synth_tile<2, 8, 64, 1, true> grid=200 block=512 args=16385,1,64,200,200,1
tile ss=2 n=260000 nb=7 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0,1 -> synth_tile<2, 8, 64, 1, true> grid=56 block=512 args=260000,8,64,56,7,8
tile ss=2 n=260000 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0,1 -> synth_tile<2, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
tile ss=2 n=2500000 nb=7 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0,1 -> synth_tile<2, 8, 64, 1, true> grid=539 block=512 args=2500000,77,64,539,7,77
tile ss=2 n=2500000 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0,1 -> synth_tile<2, 8, 64, 1, true> grid=15400 block=512 args=2500000,77,64,15400,200,77
seg ss=2 n=65 nb=7 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0,1 -> synth_tile<2, 8, 64, 1, true> grid=7 block=512 args=65,1,64,7,7,1
seg ss=2 n=65 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0,1 -> synth_tile<2, 8, 64, 1, true> grid=200 block=512 args=65,1,64,200,200,1
seg ss=2 n=16385 nb=7 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0,1 -> synth_tile<2, 8, 64, 1, true> grid=7 block=512 args=16385,1,64,7,7,1
seg ss=2 n=16385 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0,1 -> synth_tile<2, 8, 64, 1, true> grid=200 block=512 args=16385,1,64,200,200,1
seg ss=2 n=260000 nb=7 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0,1 -> synth_tile<2, 8, 64, 1, true> grid=56 block=512 args=260000,8,64,56,7,8
seg ss=2 n=260000 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0,1 -> synth_tile<2, 8, 64, 1, true> grid=1600 block=512 args=260000,8,64,1600,200,8
seg ss=2 n=2500000 nb=7 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 -> synth_tile<2, 8, 64, 1, true> grid=527 block=512 args=2500000,74,66,296,4,77
seg ss=2 n=2500000 nb=7 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=1 -> synth_tile<2, 8, 64, 1, true> grid=539 block=512 args=2500000,77,64,539,7,77
seg ss=2 n=2500000 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 -> synth_tile<2, 8, 64, 1, true> grid=6908 block=512 args=2500000,33,148,6369,193,77
seg ss=2 n=2500000 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=1 -> synth_tile<2, 8, 64, 1, true> grid=10425 block=512 args=2500000,52,94,10348,199,77
segh ss=2 n=65 nb=7 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0,1 -> synth_tile<2, 8, 32, 2, true> grid=7 block=512 args=65,1,32,7,7,1
segh ss=2 n=65 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0,1 -> synth_tile<2, 8, 32, 2, true> grid=200 block=512 args=65,1,32,200,200,1
segh ss=2 n=16385 nb=7 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0,1 -> synth_tile<2, 8, 32, 2, true> grid=14 block=512 args=16385,2,32,14,7,2
segh ss=2 n=16385 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0,1 -> synth_tile<2, 8, 32, 2, true> grid=400 block=512 args=16385,2,32,400,200,2
segh ss=2 n=260000 nb=7 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0,1 -> synth_tile<2, 8, 32, 2, true> grid=112 block=512 args=260000,16,32,112,7,16
segh ss=2 n=260000 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 -> synth_tile<2, 8, 32, 2, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segh ss=2 n=260000 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=1 -> synth_tile<2, 8, 32, 2, true> grid=3004 block=512 args=260000,15,34,2940,196,16
segh ss=2 n=2500000 nb=7 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 -> synth_tile<2, 8, 32, 2, true> grid=1051 block=512 args=2500000,148,33,592,4,153
segh ss=2 n=2500000 nb=7 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=1 -> synth_tile<2, 8, 32, 2, true> grid=1071 block=512 args=2500000,153,32,1071,7,153
segh ss=2 n=2500000 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 -> synth_tile<2, 8, 32, 2, true> grid=7080 block=512 args=2500000,33,148,6468,196,153
segh ss=2 n=2500000 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=1 -> synth_tile<2, 8, 32, 2, true> grid=10501 block=512 args=2500000,52,94,10348,199,153
segb ss=2 n=65 nb=7 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0,1 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=7 block=512 args=65,1,32,7,7,1
segb ss=2 n=65 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0,1 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=200 block=512 args=65,1,32,200,200,1
segb ss=2 n=16385 nb=7 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0,1 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=14 block=512 args=16385,2,32,14,7,2
segb ss=2 n=16385 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0,1 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=400 block=512 args=16385,2,32,400,200,2
segb ss=2 n=260000 nb=7 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0,1 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=112 block=512 args=260000,16,32,112,7,16
segb ss=2 n=260000 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=2192 block=512 args=260000,10,51,1680,168,16
segb ss=2 n=260000 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=1 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=3004 block=512 args=260000,15,34,2940,196,16
segb ss=2 n=2500000 nb=7 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=1051 block=512 args=2500000,148,33,592,4,153
segb ss=2 n=2500000 nb=7 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=1 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=1071 block=512 args=2500000,153,32,1071,7,153
segb ss=2 n=2500000 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=0 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=7080 block=512 args=2500000,33,148,6468,196,153
segb ss=2 n=2500000 nb=200 act=8 amp=1000 z=0 lv=0 scr=1 fast=1 pol=1 -> synth_tile<2, 8, 32, 1, true, 8, true> grid=10501 block=512 args=2500000,52,94,10348,199,153
auto_variant kRowsMaxCodeStep-1 -> seg
auto_variant kRowsMaxCodeStep+0 -> seg
auto_variant kRowsMaxCodeStep+1 -> segh
auto_variant kHalfRowsMaxCodeStep-1 -> segh
auto_variant kHalfRowsMaxCodeStep+0 -> segh
auto_variant kHalfRowsMaxCodeStep+1 -> generic
auto_variant 0 -> seg
scratch auto -> 0 0 0 0 0
scratch generic -> 0 0 0 0 0
scratch rows -> 0 0 0 0 0
scratch rowsx -> 0 0 0 0 0
scratch tile -> 0 0 0 0 0
scratch seg -> 0 0 0 0 0
scratch segh -> 0 0 0 0 0
scratch segm -> 104012800 128 768 0 0
scratch segb -> 0 0 0 0 0
"""


def test_launch_plans_are_the_parents(tmp_path):
    exe = str(tmp_path / "launch_plans")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "launch_plans.cpp")], check=True)
    got = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout.splitlines()
    want = EXPECTED.splitlines()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
