/* No-op OpenGL / GLU / GLUT: the reference draws finished buckets and a preview through
 * these; the reference driver (oracle/ref/ref_driver.cpp) only reads the floats its
 * renderer returns, so every call does nothing.  Our own text. */
#ifndef MRT_REF_GLUT_SHIM_H
#define MRT_REF_GLUT_SHIM_H

typedef unsigned int GLenum;
typedef unsigned int GLbitfield;
typedef int GLint;
typedef int GLsizei;
typedef float GLfloat;
typedef double GLdouble;
typedef void GLvoid;

enum {
    GL_BACK = 1, GL_FRONT, GL_FRONT_AND_BACK, GL_LIGHTING, GL_LINE, GL_MODELVIEW, GL_PROJECTION, GL_RGB,
    GL_SMOOTH, GL_TEXTURE_2D, GL_TRIANGLES, GL_UNSIGNED_BYTE,
    GL_COLOR_BUFFER_BIT = 0x4000, GL_DEPTH_BUFFER_BIT = 0x100,
    GLUT_RGB = 0, GLUT_DOUBLE = 2, GLUT_DOWN = 0, GLUT_LEFT_BUTTON = 0, GLUT_MIDDLE_BUTTON = 1,
    GLUT_RIGHT_BUTTON = 2, GLUT_KEY_UP = 101, GLUT_KEY_DOWN = 103
};

static inline void glVertex3f(GLfloat, GLfloat, GLfloat) {}
static inline void glMatrixMode(GLenum) {}
static inline void glLoadIdentity() {}
static inline void glFinish() {}
static inline void glBegin(GLenum) {}
static inline void glEnd() {}
static inline void glRasterPos2f(GLfloat, GLfloat) {}
static inline void glDrawPixels(GLsizei, GLsizei, GLenum, GLenum, const GLvoid*) {}
static inline void glReadPixels(GLint, GLint, GLsizei, GLsizei, GLenum, GLenum, GLvoid*) {}
static inline void glDrawBuffer(GLenum) {}
static inline void glDisable(GLenum) {}
static inline void glViewport(GLint, GLint, GLsizei, GLsizei) {}
static inline void glTranslatef(GLfloat, GLfloat, GLfloat) {}
static inline void glShadeModel(GLenum) {}
static inline void glPushMatrix() {}
static inline void glPopMatrix() {}
static inline void glPolygonMode(GLenum, GLenum) {}
static inline void glColor3f(GLfloat, GLfloat, GLfloat) {}
static inline void glClearColor(GLfloat, GLfloat, GLfloat, GLfloat) {}
static inline void glClear(GLbitfield) {}
static inline void gluPerspective(GLdouble, GLdouble, GLdouble, GLdouble) {}
static inline void gluLookAt(GLdouble, GLdouble, GLdouble, GLdouble, GLdouble, GLdouble, GLdouble, GLdouble, GLdouble) {}
static inline void glutWireSphere(GLdouble, GLint, GLint) {}
static inline void glutSwapBuffers() {}
static inline void glutPostRedisplay() {}
static inline void glutMainLoop() {}
static inline void glutInit(int*, char**) {}
static inline void glutInitWindowSize(int, int) {}
static inline void glutInitWindowPosition(int, int) {}
static inline void glutInitDisplayMode(unsigned int) {}
static inline int glutCreateWindow(const char*) { return 0; }
static inline void glutDisplayFunc(void (*)()) {}
static inline void glutReshapeFunc(void (*)(int, int)) {}
static inline void glutKeyboardFunc(void (*)(unsigned char, int, int)) {}
static inline void glutSpecialFunc(void (*)(int, int, int)) {}
static inline void glutMouseFunc(void (*)(int, int, int, int)) {}
static inline void glutMotionFunc(void (*)(int, int)) {}

#endif
