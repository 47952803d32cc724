#!/bin/bash
# Build oracle_arraybeam: the reference's stationbeam.c, transforms.c,
# elementbeam.c and myblas.c, unmodified, against tools/oracle/miniblas.c,
# linked with the driver in this directory. Nothing built here is kept in
# git. Usage: REF=<reference tree> bash build_oracle_beam.sh [outdir]
set -e
: "${REF:?set REF to the reference source tree}"
HERE=$(cd "$(dirname "$0")" && pwd)
OUT=${1:-$HERE/../../oracle/_ref/beam}
mkdir -p "$OUT"
CFLAGS="-O2 -fcommon -I$REF/src/lib/Dirac -I$REF/src/lib/Radio"
objs=""
for src in Radio/stationbeam.c Radio/transforms.c Radio/elementbeam.c \
           Dirac/myblas.c; do
  o="$OUT/$(basename "$src" .c).o"
  gcc $CFLAGS -c "$REF/src/lib/$src" -o "$o"
  objs="$objs $o"
done
gcc $CFLAGS -c "$HERE/../oracle/miniblas.c" -o "$OUT/miniblas.o"
gcc $CFLAGS "$HERE/oracle_arraybeam.c" $objs "$OUT/miniblas.o" \
    -lpthread -lm -o "$OUT/oracle_arraybeam"
echo "built: $OUT/oracle_arraybeam"
