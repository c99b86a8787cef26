"""The host classes' fatal path ends the process (CPU only, no device).  A failed gmg_init or upload is fatal by the reference's
convention: "ERROR: ..." on stderr, then exit (EXIT_FAILURE).  exit () runs the destructors of models in static storage -- where the
reference's CLIs keep theirs (ICM_t Gene_ICM; ICM_t Indep_Model (3, 2, 3)) -- on the thread that failed, and those destructors take
the lock of the device mirrors when they have one to drop: so no path may reach exit () with that lock held.
The three host sources are compiled as they are and linked, without the library, against stubs of every gmg_* function they
name; the stubs fail where a case says so.  Every case must print its message and exit with status 1 within the time limit."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "glimmer-mg_amd", "host")
SOURCES = ["icm.cc", "icm_train.cc", "fixed_icm.cc"]
LIMIT_S = 10                                             # a cap: the program does nothing but fail

MAIN = r"""
#include "icm.hh"
#include <stdlib.h>
#include <string.h>
int  Verbose = 0;
//  models in static storage, as in the reference's glimmer3.cc / glimmer-mg.cc: destroyed by exit ()
ICM_t  Gene_ICM (12, 7, 3);
ICM_t  Indep_Model (3, 2, 3);
Fixed_Length_ICM_t  Fixed_Model;
int  main  (int argc, char * * argv)
  {
   if  (argc > 1 && strcmp (argv [1], "fixed") == 0)
       Fixed_Model . Device_Model ();                    //  never read: fatal
   else
       Gene_ICM . Device_Model ();                       //  gmg_init or gmg_model_upload fails in the stubs: fatal
   return  0;                                            //  (not reached)
  }
"""

STUB_HEAD = r"""
#include <stdlib.h>
#include <string.h>
static int fails (const char * what)  { const char * e = getenv ("STUB_FAIL");  return  e != NULL && strcmp (e, what) == 0; }
const char * gmg_last_error (void)  { return  "the stub says no"; }
int gmg_init (int device)  { (void) device;  return  fails ("init") ? -2 : 0; }
int gmg_model_upload (void)  { return  -4; }
"""
SPECIAL = {"gmg_last_error", "gmg_init", "gmg_model_upload"}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx, cc, nm = shutil.which("g++") or shutil.which("c++"), shutil.which("gcc") or shutil.which("cc"), shutil.which("nm")
    assert cxx and cc and nm, "needs a host C++ compiler and nm"
    d = tmp_path_factory.mktemp("fatal")
    objs = []
    for src in SOURCES:
        obj = str(d / (src + ".o"))
        subprocess.run([cxx, "-std=c++17", "-O1", "-w", "-c", "-o", obj, os.path.join(HOST, src)], check=True, timeout=300)
        objs.append(obj)
    (d / "main.cc").write_text(MAIN)
    subprocess.run([cxx, "-std=c++17", "-O1", "-w", "-I", HOST, "-c", "-o", str(d / "main.o"), str(d / "main.cc")], check=True, timeout=120)
    undefined = subprocess.run([nm, "-u"] + objs, check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    names = sorted({n for n in undefined if n.startswith("gmg_")})
    assert SPECIAL <= set(names) and "gmg_model_free" in names and "gmg_fixed_model_upload" in names and len(names) > 10
    # every other entry point the host classes name: present for the link, refuses if it were called
    (d / "stubs.c").write_text(STUB_HEAD + "".join("int %s (void)  { return  -4; }\n" % n for n in names if n not in SPECIAL))
    subprocess.run([cc, "-O1", "-w", "-c", "-o", str(d / "stubs.o"), str(d / "stubs.c")], check=True, timeout=120)
    exe = str(d / "fatal")
    subprocess.run([cxx, "-pthread", "-o", exe, str(d / "main.o"), str(d / "stubs.o")] + objs, check=True, timeout=120)
    return exe


@pytest.mark.parametrize("case,args,message", [
    ("init", [], "ERROR:  gmg_init: the stub says no"),
    ("upload", [], "ERROR:  gmg_model_upload: the stub says no"),
    ("none", ["fixed"], "ERROR:  Fixed_Length_ICM_t used before read"),
])
def test_a_fatal_failure_exits_with_status_1(program, case, args, message):
    env = dict(os.environ, STUB_FAIL=case)
    try:
        res = subprocess.run([program] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=LIMIT_S)
    except subprocess.TimeoutExpired:
        pytest.fail("the program was still running after %d s: exit () was reached with the mirror lock held" % LIMIT_S)
    assert res.returncode == 1, (res.returncode, res.stderr.decode()[-300:])
    assert message in res.stderr.decode()
