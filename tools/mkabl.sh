#!/bin/bash
# Builds a NON-PRODUCT flavour of the library into tools/ab/ (never into the package directory; csrc/knobs.h lists
# the switches they read).  Neither flavour can produce a wrong result:
#   tools/mkabl.sh exp      -> tools/ab/libescoin_exp.so      -DESCOIN_EXPERIMENTS: the tuning overrides are live (tilings,
#                                                             buffers, XCD grouping, DMA spread ...)
#   tools/mkabl.sh stamps   -> tools/ab/libescoin_stamps.so   -DESCOIN_STAMPS: the above plus the in-kernel stamp profiles
#                                                             of the tiled and dense kernels (ESCOIN_PROF=1)
# ABL_CFLAGS adds flags (e.g. -DESCOIN_PROF_STARTUP), ABL_NAME overrides the output tag.  Select a flavour at run
# time with ESCOIN_LIB=$PWD/tools/ab/libescoin_<tag>.so (the Python binding; the product never reads it).
# The sources and flags are the product's: csrc/Makefile builds the flavour, with its objects under /tmp/abl_<tag>/.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
FLAVOUR=${1:-}
case $FLAVOUR in
  exp) DEF=-DESCOIN_EXPERIMENTS ;;
  stamps) DEF=-DESCOIN_STAMPS ;;
  *) echo "usage: $0 exp|stamps"; exit 2 ;;
esac
TAG=${ABL_NAME:-$FLAVOUR}
O=/tmp/abl_$TAG/
rm -rf $O
mkdir -p $O $ROOT/tools/ab
make -C $ROOT/caffe-escoin_amd/csrc -j16 OBJDIR=$O DEFS="$DEF ${ABL_CFLAGS:-}" OUT=$ROOT/tools/ab/libescoin_$TAG.so
ls -la $ROOT/tools/ab/libescoin_$TAG.so
