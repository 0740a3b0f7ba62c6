/* ops_keepsegments.c -- keepsegments (device shim).  Not an operator of the reference: the segments `segments` would list
 * -- regions above a threshold, joined across short gaps, the short and the low ones dropped -- written back into the
 * signal, so that a pipeline can go on with them: every base outside a kept segment becomes --zero, every base of a kept
 * segment (the joined gaps included) becomes --one, stays what it is, or becomes a figure of its segment (its height,
 * area, mean, length ...).  With no filters and --as=one it is binarize.
 *
 * The segments are selected by the options of `segments`, parsed by its parser, and found by its pass (segments_run,
 * ops_segments.c): a genome-wide operator on whole chromosomes, each device served once over its chromosomes.  The pass
 * paints every chromosome's partner (gdsp_keep_segments_batch, include/genodsp_hip.h) and the partner becomes the
 * signal; the table of the kept segments is written only when --output= names a file.  The variables segments, covered
 * and longest are set.
 *
 * The driver finds this operator and `segments` through opgroup_segments, at the end of this file (host_services.h). */
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include "genodsp_interface.h"
#include "genodsp_hip.h"
#include "utilities.h"
#include "host_services.h"

dspprototypes(op_keepsegments)  dspprototypes(op_segments)

typedef struct dspop_keepsegments
	{
	dspop   common;
	segments_opts  o;
	segments_paint paint;
	int     haveOne;
	} dspop_keepsegments;

OP_SHORT (op_keepsegments, "keep the regions `segments` would list: one, the signal or a figure of the region inside, zero elsewhere (not in genodsp)")

void op_keepsegments_usage (char* name, FILE* f, char* indent)
	{
	if (indent == NULL) indent = "";
	fprintf (f, "%sRewrite the signal from the regions `segments` would list for the same options: runs of bases above\n", indent);
	fprintf (f, "%sa threshold, joined across short gaps, the short and the low ones dropped. Every base outside a\n", indent);
	fprintf (f, "%skept region becomes the zero value; every base of a kept region, joined gaps included, becomes\n", indent);
	fprintf (f, "%sthe one value, keeps its value, or becomes a figure of its region. Without filters and with\n", indent);
	fprintf (f, "%s--as=one this is binarize. Sets the variables segments, covered and longest. Not in genodsp.\n\n", indent);
	fprintf (f, "%susage: %s [<threshold>] [options]\n", indent, name);
	fprintf (f, "%s  <threshold>              numeric threshold (default 0.0)\n", indent);
	fprintf (f, "%s  --threshold=<variable>   (T=) threshold from a named variable, e.g. percentile99\n", indent);
	fprintf (f, "%s  --ties:below|above       whether values equal to the threshold count as below (default) or above\n", indent);
	fprintf (f, "%s  --mergegap=<bases>       join regions no more than this many bases apart (default 0)\n", indent);
	fprintf (f, "%s  --minlength=<bases>      drop regions shorter than this, after joining (default 1)\n", indent);
	fprintf (f, "%s  --minheight=<value|variable>  drop regions whose maximum is below this\n", indent);
	fprintf (f, "%s  --as=one|value|count|length|sum|mean|min|max\n", indent);
	fprintf (f, "%s                           what a base of a kept region becomes: the one value (default), its own\n", indent);
	fprintf (f, "%s                           value, or that figure of its region as `segments` prints it\n", indent);
	fprintf (f, "%s  --one=<value>            (O=) the one value (default 1.0; only with --as=one)\n", indent);
	fprintf (f, "%s  --zero=<value>           (Z=) what a base outside every kept region becomes (default 0.0)\n", indent);
	fprintf (f, "%s  --output=<file>          also write the table of the kept regions there, as `segments` writes it\n", indent);
	fprintf (f, "%s  --precision=<number>     digits after the point in that table (default: all of them)\n", indent);
	fprintf (f, "%s  --origin=one|zero        coordinate convention of the positions in that table\n", indent);
	}

dspop* op_keepsegments_parse (char* name, int argc, char** argv)
	{
	static const char* modes[] = { "one", "value", "count", "length", "sum", "mean", "min", "max" };      /* GDSP_KEEP_* */
	dspop_keepsegments* op = (dspop_keepsegments*) new_op (name, sizeof(dspop_keepsegments), true);
	segments_opts_init (&op->o);
	op->paint.mode = GDSP_KEEP_ONE;  op->paint.one = 1.0;  op->paint.zero = 0.0;
	for ( ; argc > 0 ; argv++, argc--)
		{
		char* arg = argv[0];
		char* argVal = strchr (arg, '=');  if (argVal != NULL) argVal++;
		if (segments_opts_take (&op->o, name, arg)) continue;
		if (strcmp_prefix (arg, "--as=") == 0)
			{
			int mode = -1;
			for (int k=0 ; k<(int) (sizeof(modes)/sizeof(modes[0])) ; k++) { if (strcmp (argVal, modes[k]) == 0) mode = k; }
			if (mode < 0) chastise ("[%s] --as must be one of one, value, count, length, sum, mean, min, max (\"%s\")\n", name, arg);
			op->paint.mode = mode;
			continue;
			}
		if (is_opt3 (arg, "one", "O"))  { op->paint.one  = string_to_valtype (argVal);  op->haveOne = true;  continue; }
		if (is_opt3 (arg, "zero", "Z")) { op->paint.zero = string_to_valtype (argVal);  continue; }
		segments_opts_take_other (&op->o, name, arg);
		}
	if (op->haveOne && (op->paint.mode != GDSP_KEEP_ONE))
		chastise ("[%s] --one goes with --as=one only (--as=%s writes the region's own %s)\n", name, modes[op->paint.mode], modes[op->paint.mode]);
	/* (a number given here is known now; one that comes from a variable is looked at when the operator runs) */
	if ((op->o.thresholdVarName == NULL) && (op->o.threshold != op->o.threshold)) chastise ("[%s] the threshold is not a number\n", name);
	if (op->o.haveMinHeight && (op->o.minHeightVarName == NULL) && (op->o.minHeight != op->o.minHeight))
		chastise ("[%s] the minimum height is not a number\n", name);
	return (dspop*) op;
	}

void op_keepsegments_free (dspop* _op)
	{
	dspop_keepsegments* op = (dspop_keepsegments*) _op;
	segments_opts_free (&op->o);
	free (op);
	}

void op_keepsegments_apply (dspop* _op, arg_dont_complain(char* vName), arg_dont_complain(u32 vLen), arg_dont_complain(valtype* v))
	{
	dspop_keepsegments* op = (dspop_keepsegments*) _op;
	segments_run (_op, &op->o, op->o.outFilename != NULL, &op->paint);
	}

/* the driver: both work on whole chromosomes.  segments only reads the signal (and the tiles that hold regions);
 * keepsegments adds a store per base through the partners and, with --as=value, the signal again inside the regions */
static void segments_work (dspop* op, u64* bases, double* bytesPerBase) { *bytesPerBase = 8; }
static void keepsegments_work (dspop* op, u64* bases, double* bytesPerBase)
	{ *bytesPerBase = (((dspop_keepsegments*) op)->paint.mode == GDSP_KEEP_VALUE)? 24 : 16; }

static const dspinfo segmentsRows[] =
	{ dspinforecord("segments"    , op_segments)    , dspinfoalias ("callpeaks")    , dspinfoalias ("call_peaks"), dspinfoalias ("islands"),
	  dspinforecord("keepsegments", op_keepsegments), dspinfoalias ("keep_segments"), dspinfoalias ("hysteresis"), dspinfoalias ("paintsegments") };
static const optraits segmentsTraits[] =
	{ { op_segments_apply,     true,  false, NULL, NULL, segments_work },
	  { op_keepsegments_apply, false, false, NULL, NULL, keepsegments_work } };
const opgroup opgroup_segments = OPGROUP (segmentsRows, segmentsTraits, NULL);
