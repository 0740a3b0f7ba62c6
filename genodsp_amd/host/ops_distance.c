/* ops_distance.c -- distance (device shim).  Not an operator of the reference: every base becomes its distance, in bases,
 * to the nearest base above a threshold -- the figure under dilate and erode (ops_morphology.c), which each answer one
 * radius of it.  The threshold is given as `segments` takes it (ops_segments.c parses it for both).
 * The definition is at gdsp_distance (include/genodsp_hip.h).
 *
 * The driver finds this operator through opgroup_distance, at the end of this file (host_services.h); every call into the
 * device library for it stays here. */
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include "genodsp_interface.h"
#include "genodsp_hip.h"
#include "utilities.h"
#include "host_services.h"

dspprototypes(op_distance)

typedef struct dspop_distance
	{
	dspop   common;
	segments_opts o;                                               /* the threshold and its ties; nothing else of it is used */
	int     to;                                                    /* GDSP_DISTANCE_* */
	int     isSigned;
	u32     cap;                                                   /* 0: none */
	} dspop_distance;

OP_SHORT (op_distance, "replace each base by its distance to the nearest base above a threshold (not in genodsp)")

void op_distance_usage (char* name, FILE* f, char* indent)
	{
	if (indent == NULL) indent = "";
	fprintf (f, "%sReplace every base by its distance, in bases, to the nearest base whose value is above a\n", indent);
	fprintf (f, "%sthreshold; such a base gets 0, its neighbour 1. Where a chromosome has no such base on the side(s)\n", indent);
	fprintf (f, "%sasked for, the result is the chromosome's length, which no distance reaches. dilate and\n", indent);
	fprintf (f, "%serode answer one radius of this each: `= distance --max=R = binarize r` inverted is the\n", indent);
	fprintf (f, "%sdilation by r on both sides, for every r below R. Not in genodsp.\n\n", indent);
	fprintf (f, "%susage: %s [<threshold>] [options]\n", indent, name);
	fprintf (f, "%s  <threshold>              numeric threshold (default 0.0)\n", indent);
	fprintf (f, "%s  --threshold=<variable>   (T=) threshold from a named variable, e.g. percentile99\n", indent);
	fprintf (f, "%s  --ties:below|above       whether values equal to the threshold count as below (default) or above\n", indent);
	fprintf (f, "%s  --to=nearest             the distance to the nearest such base on either side\n", indent);
	fprintf (f, "%s                           (this is the default)\n", indent);
	fprintf (f, "%s  --to=left                the distance to the nearest one at lower coordinates\n", indent);
	fprintf (f, "%s  --to=right               the distance to the nearest one at higher coordinates\n", indent);
	fprintf (f, "%s  --signed                 bases above the threshold get minus their distance to the nearest\n", indent);
	fprintf (f, "%s                           base that is not (the chromosome's ends count as such): the depth\n", indent);
	fprintf (f, "%s                           inside a region, -1 at its edges; nothing is 0 then\n", indent);
	fprintf (f, "%s  --max=<bases>            no result beyond this many bases, either sign (e.g. 10K); a base with\n", indent);
	fprintf (f, "%s                           nothing on the side asked for gets this too\n", indent);
	}

dspop* op_distance_parse (char* name, int argc, char** argv)
	{
	dspop_distance* op = (dspop_distance*) new_op (name, sizeof(dspop_distance), false);
	segments_opts_init (&op->o);
	op->to = GDSP_DISTANCE_NEAREST;
	for ( ; argc > 0 ; argv++, argc--)
		{
		char* arg = argv[0];
		char* argVal = strchr (arg, '=');  if (argVal != NULL) argVal++;
		if (segments_threshold_take (&op->o, name, arg)) continue;
		if (strcmp_prefix (arg, "--to=") == 0)
			{
			if      (strcmp (argVal, "nearest") == 0) op->to = GDSP_DISTANCE_NEAREST;
			else if (strcmp (argVal, "left")    == 0) op->to = GDSP_DISTANCE_LEFT;
			else if (strcmp (argVal, "right")   == 0) op->to = GDSP_DISTANCE_RIGHT;
			else chastise ("[%s] --to must be nearest, left or right (\"%s\")\n", name, arg);
			continue;
			}
		if (strcmp (arg, "--signed") == 0) { op->isSigned = true;  continue; }
		if (strcmp_prefix (arg, "--max=") == 0)
			{
			int r = string_to_unitized_int (argVal, /*thousands*/ true);
			if (r == 0) chastise ("[%s] --max can't be zero (\"%s\")\n", name, arg);
			if (r < 0)  chastise ("[%s] --max can't be negative (\"%s\")\n", name, arg);
			op->cap = (u32) r;
			continue;
			}
		segments_opts_take_other (&op->o, name, arg);              /* --debug, an option nobody knows, the threshold */
		}
	return (dspop*) op;
	}

void op_distance_free (dspop* _op)
	{
	dspop_distance* op = (dspop_distance*) _op;
	segments_opts_free (&op->o);
	free (op);
	}

/* the variable is fetched when the operator first runs: by then `percentile` or `stats` has set it */
static void resolve_threshold (dspop_distance* op)
	{
	resolve_variable (&op->common, &op->o.thresholdVarName, &op->o.threshold, "threshold");
	if (op->o.threshold != op->o.threshold)
		{ fprintf (stderr, "[%s] the threshold is not a number\n", op->common.name);  exit (EXIT_FAILURE); }
	}

void op_distance_apply (dspop* _op, arg_dont_complain(char* vName), u32 vLen, valtype* v)
	{
	dspop_distance* op = (dspop_distance*) _op;
	resolve_threshold (op);
	check_gdsp (gdsp_distance (v, vLen, op->o.threshold, op->o.tiesAbove, op->to, op->isSigned, op->cap, op_stream ()), _op->name);
	}

/* the driver: with --max=R a base depends on the R bases to either side of it and on nothing else; without, on its whole
 * chromosome, which then stays in one piece under --sharding=bases.  One launch sequence per device */
static int distance_reach (dspop* _op, u32* left, u32* right)
	{
	dspop_distance* op = (dspop_distance*) _op;
	if (op->cap == 0) return false;
	*left = *right = op->cap;
	return true;
	}

static int distance_batch (dspop* _op, const gdsp_batch_item* items, int nitems, void* stream)
	{
	dspop_distance* op = (dspop_distance*) _op;
	resolve_threshold (op);
	return gdsp_distance_batch (items, nitems, op->o.threshold, op->o.tiesAbove, op->to, op->isSigned, op->cap, stream);
	}

static const dspinfo distanceRows[] =
	{ dspinforecord("distance", op_distance), dspinfoalias ("distancetransform"), dspinfoalias ("distance_transform"),
	  dspinfoalias ("nearest") };
static const optraits distanceTraits[] = { { op_distance_apply, true, false, distance_reach, distance_batch, NULL } };
const opgroup opgroup_distance = OPGROUP (distanceRows, distanceTraits, NULL);
